"""Independent model of kid_db_read_segment_votes*: segments called by root-path votes.

numpy and the oracle binding only, on top of tests/read_segments_model.py (the geometry: SegmentModel.segments) and
tests/read_votes_model.py (the rule: VoteModel).  The record of segment j of a read is (pos, n_pos) of the segment and
the kid_vote record of the read with the range [pos, pos + n_pos + k - 2].

Two forms, held against each other by tests/test_read_segment_votes_model.py:
  SegmentVoteModel.literal  builds the batch of sub-reads on copied text and calls HitModel.batch and
                            VoteModel.batch_literal on it: the defining sentence, literally
  SegmentVoteModel.direct   slices the read's hits by pos, counts the valid windows and applies the rule to the
                            slice's targets as {target: count} (read_weighted)
"""
from collections import Counter

import numpy as np

from read_segments_model import SegmentModel
from read_support_model import passes
from read_votes_model import VOTE_DTYPE, VoteModel

SEGMENT_VOTE_DTYPE = np.dtype([("pos", np.uint32), ("n_pos", np.uint32)] + [(f, np.uint32) for f in VOTE_DTYPE.names])
VOTE_FIELDS = VOTE_DTYPE.names


class SegmentVoteModel(SegmentModel):
    """one batch of reads (as SegmentModel) and its segment votes"""

    def __init__(self, support_model, bases, offsets, start=None, stop=None, keep=None):
        super().__init__(support_model, bases, offsets, start, stop, keep)
        self.vm = VoteModel(support_model)
        self._vmemo = {}

    # ---- (a) the defining sentence: every segment a read of its own, on copied text
    def literal(self, seg_len, seg_step, rule):
        off, read_of, pos, n_pos = self.segments(seg_len, seg_step)
        subs = [bytes(self.read(int(r))[int(p):int(p + m + self.k - 1)]) for r, p, m in zip(read_of, pos, n_pos)]
        text = np.frombuffer(b"".join(subs), np.uint8).copy()
        sub_off = np.zeros(len(subs) + 1, np.uint64)
        sub_off[1:] = np.cumsum([len(s) for s in subs])
        rec = self.vm.batch_literal(self.hm.batch(text, sub_off), rule)
        out = np.zeros(len(subs), SEGMENT_VOTE_DTYPE)
        out["pos"], out["n_pos"] = pos, n_pos
        for f in VOTE_FIELDS:
            out[f] = rec[f]
        return off, out

    # ---- (b) the read's own hits sliced by pos
    def direct(self, seg_len, seg_step, rule):
        hits, valid = self._whole()
        off, read_of, pos, n_pos = self.segments(seg_len, seg_step)
        out = np.zeros(pos.size, SEGMENT_VOTE_DTYPE)
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
                w = Counter(ht[h_lo[j]:h_hi[j]].tolist())  # (the record is a function of the multiset)
                key = (tuple(sorted(w.items())), int(nk[j]), rule)
                got = self._vmemo.get(key)
                if got is None:
                    got = self._vmemo[key] = self.read_weighted(w, int(nk[j]), rule)
                for f, v in zip(VOTE_FIELDS, got):
                    out[f][a + j] = v
        return off, out

    def read_weighted(self, w, n, rule):
        """VoteModel.read_literal for a multiset given as {target: count}: a segment of a long record has hundreds of
        hits and a handful of distinct targets"""
        m = sum(w.values())
        path = {c: self.vm.root_path(c) for c in w}
        p = {c: sum(w.get(a, 0) for a in path[c]) for c in w}
        best = max(p.values())
        members = [c for c in w if p[c] == best]
        common = set(path[members[0]]).intersection(*[set(path[c]) for c in members[1:]])
        call = next(a for a in path[members[0]] if a in common)  # the deepest: the path runs upwards
        s_of = lambda c: sum(k for t, k in w.items() if c in path[t])  # noqa: E731
        s_call = s_of(call)
        for c in self.vm.root_path(call):
            s = s_of(c)
            if passes(s, n, rule):
                return (call, c, n, m, best, len(members), s_call, s)
        return (call, 0, n, m, best, len(members), s_call, 0)


def segment_votes_line(final, trimmed_len, records, header):
    """a read's line of a segment_votes file (bytes; header: bytes), or b"" when none of its segments holds a hit"""
    with_hit = [s for s in records if s["n_hits"] > 0]
    if not with_hit:
        return b""
    cols = b" ".join(b"%d:%d:%d:%d:%d:%d:%d:%d" % (s["pos"], s["n_pos"], s["n_kmers"], s["n_hits"], s["call"], s["confident"], s["p_best"],
                                                   s["n_best"]) for s in with_hit)
    return b"%d\t%d\t%d\t%d\t%s\t%s\n" % (final, trimmed_len, len(records), len(with_hit), cols, header)
