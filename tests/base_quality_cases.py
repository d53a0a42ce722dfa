"""Inputs and numpy expectations shared by the tests of --min-base-quality / KID_OPT_MIN_BASE_QUALITY: bases whose
quality byte, read as signed char, is below Q + 33 are read as 'N'.  numpy and the oracle only -- nothing from the code
under test decides an expectation."""
import numpy as np

from helpers import K, synth
from read_hits_model import HitModel

LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 29, 30, 31, 63, 64, 65, 150, 250, 257]
LONG = 70001
# around every threshold the tests use (Q = 1, 2, 20, 40, 93 -> T = 34, 35, 53, 73, 126), '!' and '~', and bytes >= 128
QUAL_BYTES = np.array([33, 34, 35, 36, 52, 53, 54, 72, 73, 74, 125, 126, 127, 0x80, 0xFF], np.uint8)


def np_mask(seq, qual, q):
    """the rule in numpy -> (masked copy, bases masked)"""
    out = np.array(seq, np.uint8, copy=True)
    m = np.asarray(qual, np.uint8).view(np.int8) < q + 33
    out[m] = ord("N")
    return out, int(m.sum())


def kernel_case(seed=11):
    """reads laid back to back without a gap: the length set once per start alignment mod 16 (a read of 0..15 bases in
    front of every repetition moves it there), then one long read at an odd address -> (bases, quals, offsets).  The
    first and the last base of many reads are low-quality ('!') between high-quality ('~') bases of the adjoining reads."""
    rng = np.random.default_rng(seed)
    lens, total = [], 0
    for a in range(16):
        pad = (a - total) % 16
        lens += [pad] + LENGTHS
        total += pad + sum(LENGTHS)
    lens += [(5 - total) % 16, LONG]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    bases = rng.choice(np.frombuffer(b"ACGTACGTACGTacgtN", np.uint8), n)
    quals = rng.choice(QUAL_BYTES, n)
    edge = [i for i in range(1, len(lens) - 1) if lens[i] >= 2 and lens[i - 1] >= 2 and lens[i + 1] >= 2 and i % 2 == 0]
    for i in edge:  # high-quality neighbours first, then the low-quality ends
        quals[int(off[i]) - 1] = ord("~")
        quals[int(off[i + 1])] = ord("~")
    for i in edge:
        quals[int(off[i])] = ord("!")
        quals[int(off[i + 1]) - 1] = ord("!")
    starts = {(int(off[i]) % 16, lens[i]) for i in range(len(lens))}
    assert all((a, L) in starts for a in range(16) for L in LENGTHS if L), "every length at every start alignment"
    assert len(edge) > 50 and int(off[-2]) % 2 == 1
    return bases, quals, off


def build_block(records, aligns=None, crlf_every=0, blank_every=0):
    """FASTQ text of records [(seq, qual)] (bytes) with its line index -> (text uint8[], recs uint32[n, 4]).
    aligns[i] = (a, b): the header and the '+' line of record i are padded until seq_off % 16 == a and
    qual_off % 16 == b.  crlf_every: every crlf_every-th record ends its lines with CR LF; blank_every: blank lines
    (with and without CR) behind every blank_every-th record."""
    text, recs = bytearray(), []
    for i, (s, q) in enumerate(records):
        eol = b"\r\n" if crlf_every and i % crlf_every == 0 else b"\n"
        head, plus = b"@r%d" % i, b"+"
        if aligns is not None and aligns[i] is not None:
            a, b = aligns[i]
            head += b"h" * ((a - (len(text) + len(head) + len(eol))) % 16)
            plus += b"p" * ((b - (len(text) + len(head) + len(eol) + len(s) + len(eol) + len(plus) + len(eol))) % 16)
        text += head + eol
        so = len(text)
        text += bytes(s) + eol + plus + eol
        qo = len(text)
        text += bytes(q) + eol
        if blank_every and i % blank_every == 0:
            text += b"\r\n\n"
        recs.append((so, len(s), qo, len(q)))
    return np.frombuffer(bytes(text), np.uint8), np.array(recs, np.uint32).reshape(-1, 4)


def mask_block(text, recs, q):
    """the block with the masked bases of every record with qual_len >= seq_len replaced by 'N' -> (text, bases masked)"""
    out, n = np.array(text, np.uint8, copy=True), 0
    for so, sl, qo, ql in np.asarray(recs).tolist():
        if ql < sl:
            continue
        m = text[qo:qo + sl].view(np.int8) < q + 33
        out[so:so + sl][m] = ord("N")
        n += int(m.sum())
    return out, n


def records_of(text, recs):
    raw = bytes(text)
    return ([raw[so:so + sl] for so, sl, qo, ql in np.asarray(recs).tolist()],
            [raw[qo:qo + ql] for so, sl, qo, ql in np.asarray(recs).tolist()])


def hit_reads(odb, keys, targets, parent, cum, n, r0, u_is_t=False):
    """n reads of 150 bases that have hits per the oracle, quality 'I' everywhere but for '2' -- not trimmed by
    process_qual, masked at Q = 20 -- inside hit windows: even reads get one '2', in the middle of their first hit
    window; odd reads one at the last base of every hit window that holds none yet -> [(seq, qual)]"""
    L = 150
    bases = synth.reads(cum, parent, 3 * n, L, K, r0=r0)
    off = synth.fixed_offsets(3 * n, L)
    hits = HitModel(odb, keys, targets, K, u_is_t=u_is_t).batch(bases, off)
    out = []
    for r in range(3 * n):
        pos = hits.of(r)[0].tolist()
        if not pos:
            continue
        q = np.full(L, ord("I"), np.uint8)
        if len(out) % 2 == 0:
            q[pos[0] + K // 2] = ord("2")
        else:
            for p in pos:
                if not (q[p:p + K] == ord("2")).any():
                    q[p + K - 1] = ord("2")
        out.append((bases[r * L:(r + 1) * L].tobytes(), q.tobytes()))
        if len(out) == n:
            break
    assert len(out) == n, "too few synthetic reads with hits"
    return out


def block_records(odb, keys, targets, parent, cum, n_synth=3000, n_hit=240):
    """the records of the FASTQ block tests -> ([(seq, qual)], aligns)"""
    rng = np.random.default_rng(5)
    L = 150
    b = synth.reads(cum, parent, n_synth, L, K, r0=777).reshape(n_synth, L)
    q = synth.qualities(n_synth, L, r0=777)
    recs = [(b[i].tobytes(), q[i].tobytes()) for i in range(n_synth)]
    recs += hit_reads(odb, keys, targets, parent, cum, n_hit, r0=90000)
    # every length of the kernel's list, cut from synthetic reads laid end to end, with mixed qualities
    pool = synth.reads(cum, parent, 480, L, K, r0=120000).tobytes()
    mixed = np.frombuffer(b"IIIIIIIIIIIIJH52#!\"", np.uint8)
    at = 0
    for ln in LENGTHS + [LONG]:
        recs.append((pool[at:at + ln], rng.choice(mixed, ln).tobytes()))
        at = (at + ln) % 1000
    aligns = [None] * len(recs)
    # seq_off mod 16 x qual_off mod 16: all 256 combinations, independently
    b2 = synth.reads(cum, parent, 256, L, K, r0=130000).reshape(256, L)
    q2 = synth.qualities(256, L, r0=5)
    for i in range(256):
        ql = q2[i].copy()
        ql[40 + i % 60] = ord("2")
        recs.append((b2[i].tobytes(), ql.tobytes()))
        aligns.append((i % 16, i // 16))
    b3 = synth.reads(cum, parent, 120, L, K, r0=140000).reshape(120, L)
    q3 = np.full((120, L), ord("I"), np.uint8)
    q3[:, 70] = ord("2")
    q3[:, 71] = ord("+")
    q3[:, 72] = ord('"')  # (masked at Q = 2 already)
    for i in range(120):
        s, ql = b3[i].tobytes(), q3[i].tobytes()
        kind = i % 4
        if kind == 0:
            ql += b"IIII##!!"  # a quality line longer than its sequence: the extra bytes are ignored
        elif kind == 1:
            s = s.lower()
        elif kind == 2:
            s = s[:20] + b"N" + s[21:100] + b"NN" + s[102:]
        else:
            s = s.replace(b"T", b"U").replace(b"t", b"u")  # bases to a KID_FLAG_U_IS_T database alone
        recs.append((s, ql))
        aligns.append(None)
    return recs, aligns
