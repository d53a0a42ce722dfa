"""Independent model of kid_db_read_segments*: records called in segments.

numpy and the oracle binding only, on top of tests/read_hits_model.py and tests/read_support_model.py.  For one read
with the trimmed range [start, stop] and P = max(0, stop - start + 1 - (k - 1)) window positions:

  n_seg      0 if P = 0, 1 if P <= seg_len, else 1 + ceil((P - seg_len) / seg_step)
  segment j  covers the positions [j * seg_step, min(j * seg_step + seg_len, P)); pos = start + j * seg_step
  its record the kid_support record of the read with the range [pos, pos + n_pos + k - 2]

Two forms, held against each other by tests/test_read_segments_model.py:
  SegmentModel.literal  builds the batch of sub-reads on copied text and calls HitModel.batch and
                        SupportModel.batch_literal on it: the defining sentence, literally
  SegmentModel.direct   slices the read's hits by pos and counts the valid windows of read_hits_model.windows
"""
import numpy as np

from read_hits_model import windows
from read_support_model import SUPPORT_DTYPE

SEGMENT_DTYPE = np.dtype([("pos", np.uint32), ("n_pos", np.uint32)] + [(f, np.uint32) for f in SUPPORT_DTYPE.names])
MAX_OVERLAP = 1024


def geometry(P, seg_len, seg_step):
    """-> (first position, positions covered) of every segment of a read with P positions, as int64 arrays"""
    assert seg_len >= 1 and 1 <= seg_step <= seg_len <= MAX_OVERLAP * seg_step
    if P <= 0:
        n = 0
    elif P <= seg_len:
        n = 1
    else:
        n = 1 + -(-(P - seg_len) // seg_step)
    q = np.arange(n, dtype=np.int64) * seg_step
    return q, np.minimum(q + seg_len, P) - q


class SegmentModel:
    """one batch of reads (host buffers; keep[r] = False: a FASTQ record process_qual drops) and its segments"""

    def __init__(self, support_model, bases, offsets, start=None, stop=None, keep=None):
        self.sm, self.hm = support_model, support_model.hm
        self.k = self.hm.k
        self.bases = np.asarray(bases, np.uint8)
        self.offsets = np.asarray(offsets, np.uint64)
        n = self.offsets.size - 1
        lens = np.diff(self.offsets.astype(np.int64))
        self.start = np.zeros(n, np.int64) if start is None else np.asarray(start, np.int64)
        self.stop = lens - 1 if stop is None else np.asarray(stop, np.int64)
        self.P = np.maximum(0, self.stop - self.start + 1 - (self.k - 1))
        if keep is not None:
            self.P = np.where(np.asarray(keep, bool), self.P, 0)
        self.n = n

    def read(self, r):
        return self.bases[int(self.offsets[r]):int(self.offsets[r + 1])]

    def segments(self, seg_len, seg_step):
        """-> CSR offsets, and per segment its read, pos and n_pos"""
        geo = [geometry(int(self.P[r]), seg_len, seg_step) for r in range(self.n)]
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum([g[0].size for g in geo])
        read_of = np.repeat(np.arange(self.n), [g[0].size for g in geo])
        pos = np.concatenate([g[0] + self.start[r] for r, g in enumerate(geo)]) if self.n else np.empty(0, np.int64)
        n_pos = np.concatenate([g[1] for g in geo]) if self.n else np.empty(0, np.int64)
        return off, read_of, pos.astype(np.int64), n_pos.astype(np.int64)

    # ---- (a) the defining sentence: every segment a read of its own, on copied text
    def literal(self, seg_len, seg_step, rule):
        off, read_of, pos, n_pos = self.segments(seg_len, seg_step)
        subs = [bytes(self.read(int(r))[int(p):int(p + m + self.k - 1)]) for r, p, m in zip(read_of, pos, n_pos)]
        text = np.frombuffer(b"".join(subs), np.uint8).copy()
        sub_off = np.zeros(len(subs) + 1, np.uint64)
        sub_off[1:] = np.cumsum([len(s) for s in subs])
        hits = self.hm.batch(text, sub_off)
        rec = self.sm.batch_literal(hits, rule, self.sm.finals(hits))
        out = np.zeros(len(subs), SEGMENT_DTYPE)
        out["pos"], out["n_pos"] = pos, n_pos
        for f in SUPPORT_DTYPE.names:
            out[f] = rec[f]
        return off, out

    # ---- (b) the read's own hits sliced by pos
    def _whole(self):
        if not hasattr(self, "_hits"):
            keep = self.P > 0
            st = np.where(keep, self.start, 0).astype(np.int32)
            sp = np.where(keep, self.stop, -1).astype(np.int32)  # (an empty range: no window)
            self._hits = self.hm.batch(self.bases, self.offsets, st, sp)
            self._valid = [windows(self.read(r), int(st[r]), int(sp[r]), self.k, self.hm.code)[1] for r in range(self.n)]
            self._memo = {}
        return self._hits, self._valid

    def direct(self, seg_len, seg_step, rule):
        hits, valid = self._whole()
        off, read_of, pos, n_pos = self.segments(seg_len, seg_step)
        out = np.zeros(pos.size, SEGMENT_DTYPE)
        out["pos"], out["n_pos"] = pos, n_pos
        for r in range(self.n):
            a, b = int(off[r]), int(off[r + 1])
            if a == b:
                continue
            hp, ht, _ = hits.of(r)
            lo, hi = pos[a:b], pos[a:b] + n_pos[a:b]
            nk = np.searchsorted(valid[r], hi) - np.searchsorted(valid[r], lo)
            h_lo, h_hi = np.searchsorted(hp, lo), np.searchsorted(hp, hi)
            out["n_kmers"][a:b] = nk
            out["n_hits"][a:b] = h_hi - h_lo
            for j in np.flatnonzero(h_hi > h_lo):
                tg = tuple(ht[h_lo[j]:h_hi[j]].tolist())
                key = (tg, int(nk[j]), rule)
                got = self._memo.get(key)
                if got is None:
                    got = self._memo[key] = self.sm.read_literal(list(tg), int(nk[j]), rule, self.hm.fold(tg))
                for f, v in zip(("final", "confident", "s_final", "s_confident"), (got[0], got[1], got[4], got[5])):
                    out[f][a + j] = v
        return off, out


def segments_line(final, trimmed_len, records, header):
    """a read's line of a segments file (bytes; header: bytes), or b"" when none of its segments holds a hit"""
    with_hit = [s for s in records if s["n_hits"] > 0]
    if not with_hit:
        return b""
    cols = b" ".join(b"%d:%d:%d:%d:%d:%d" % (s["pos"], s["n_pos"], s["n_kmers"], s["n_hits"], s["final"], s["confident"]) for s in with_hit)
    return b"%d\t%d\t%d\t%d\t%s\t%s\n" % (final, trimmed_len, len(records), len(with_hit), cols, header)
