"""Independent model of kid_db_read_hits*: every read's k-mer hits in read-position order.

numpy and the oracle binding only -- nothing from the code under test.  A hit is a k-mer window for which
Hashtable::getHash returns a target > 0, i.e. exactly the values process_read folds (newkmer_10nx.cpp:526-595):

  * keyF / keyR roll over seq[start..stop]; a byte that is not ACGTacgt (Uu under KO_FLAG_U_IS_T) resets the window
    (cpos = 0, :520-524); after a full window cpos-- (:604), so a window is full exactly when its k bytes are bases
  * the key handed to getHash is min(keyF, keyR) (:528); the target comes from OracleDB.get (probe cap included)
  * entry = index of the key's first occurrence in the `keys` array handed to the builder (targets 0 leave no cell)
  * pos = i - k + 1 for the window that ends at byte i of the read

HitModel.read_rolling is the literal loop; HitModel.batch is the same thing vectorised (tests/test_read_hits_model.py
holds the two against each other and both against the oracle's own fold and counters).
"""
import numpy as np

from oracle import binding as ob

_CODE = np.full(256, -1, np.int8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i
_CODE_U = _CODE.copy()
_CODE_U[ord("U")] = 3
_CODE_U[ord("u")] = 3


def windows(seq, start, stop, k, code=_CODE):
    """canonical keys and positions (within the read) of the full windows of seq[start..stop]"""
    nwin = stop - start + 1 - (k - 1)
    if start > stop or nwin <= 0:
        return np.empty(0, np.uint64), np.empty(0, np.int64)
    c = code[np.frombuffer(bytes(seq[start:stop + 1]), np.uint8)].astype(np.int64)
    bad = np.concatenate(([0], np.cumsum(c < 0)))
    full = (bad[k:] - bad[:nwin]) == 0
    cu = np.where(c < 0, 0, c).astype(np.uint64)
    kf = np.zeros(nwin, np.uint64)
    kr = np.zeros(nwin, np.uint64)
    for j in range(k):
        kf = (kf << np.uint64(2)) | cu[j:j + nwin]
        kr = (kr << np.uint64(2)) | (np.uint64(3) - cu[k - 1 - j:k - 1 - j + nwin])
    return np.minimum(kf, kr)[full], np.flatnonzero(full) + start


class Hits:
    """CSR result: offsets uint64[n + 1]; n_kmers uint32[n]; pos / target / entry uint32[offsets[n]]"""

    def __init__(self, offsets, n_kmers, pos, target, entry):
        self.offsets, self.n_kmers, self.pos, self.target, self.entry = offsets, n_kmers, pos, target, entry

    def of(self, r):
        a, b = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.pos[a:b], self.target[a:b], self.entry[a:b]


class HitModel:
    def __init__(self, odb, keys, targets, k, u_is_t=False):
        self.odb, self.k = odb, int(k)
        self.code = _CODE_U if u_is_t else _CODE
        keys = np.asarray(keys, np.uint64)
        live = np.flatnonzero(np.asarray(targets) != 0)  # an entry with target 0 leaves its cell empty
        self.ukeys, first = np.unique(keys[live], return_index=True)
        self.first = live[first].astype(np.uint32)

    def entry_of(self, key_array):
        i = np.searchsorted(self.ukeys, key_array)
        assert np.array_equal(self.ukeys[i], key_array), "a hit whose key is not among the builder's entries"
        return self.first[i]

    # ---- the reference's loop, byte by byte
    def read_rolling(self, seq, start, stop):
        """-> (windows looked up, [(pos, target, entry)])"""
        k, mask = self.k, (1 << (2 * self.k)) - 1
        cpos = keyF = keyR = 0
        n, out = 0, []
        for i in range(start, stop + 1):
            c = int(self.code[seq[i]])
            if c < 0:
                cpos = keyF = keyR = 0
                continue
            keyF = ((keyF << 2) & mask) | c
            keyR = (keyR >> 2) | ((3 - c) << (2 * (k - 1)))
            cpos += 1
            if cpos == k:
                key = min(keyF, keyR)
                n += 1
                t = int(self.odb.get(np.array([key], np.uint64))[0])
                if t > 0:
                    out.append((i - k + 1, t, int(self.entry_of(np.array([key], np.uint64))[0])))
                cpos -= 1
        return n, out

    # ---- the same, vectorised per read; one oracle call per batch
    def _windows(self, seq, start, stop):
        return windows(seq, start, stop, self.k, self.code)

    def batch(self, bases, offsets, start=None, stop=None):
        bases = np.asarray(bases, np.uint8)
        offsets = np.asarray(offsets, np.uint64)
        n = offsets.size - 1
        keys, poss, counts = [], [], np.zeros(n, np.int64)
        for r in range(n):
            a, b = int(offsets[r]), int(offsets[r + 1])
            s0 = 0 if start is None else int(start[r])
            e0 = b - a - 1 if stop is None else int(stop[r])
            key, pos = self._windows(bases[a:b], s0, e0)
            keys.append(key)
            poss.append(pos)
            counts[r] = key.size
        key = np.concatenate(keys) if keys else np.empty(0, np.uint64)
        pos = np.concatenate(poss) if poss else np.empty(0, np.int64)
        tgt = self.odb.get(key) if key.size else np.empty(0, np.uint32)
        hit = tgt > 0
        read_of = np.repeat(np.arange(n), counts)
        per_read = np.bincount(read_of[hit], minlength=n) if n else np.zeros(0, np.int64)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(per_read)
        return Hits(off, counts.astype(np.uint32), pos[hit].astype(np.uint32), tgt[hit].astype(np.uint32),
                    self.entry_of(key[hit]).astype(np.uint32) if hit.any() else np.empty(0, np.uint32))

    def fold(self, targets):
        """process_read's left fold over a read's hit targets (newkmer_10nx.cpp:588-595); msca is not associative"""
        f = 0
        for t in targets:
            t = int(t)
            f = self.odb.msca(t, f) if f > 0 else t
        return f


def trim_ranges(quals, seq_lens, k):
    """process_qual per read via the oracle -> (start, stop, keep); keep = the reference calls process_read"""
    n = len(quals)
    start, stop, keep = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, bool)
    for r in range(n):
        called, st, sp = ob.process_qual(quals[r], int(seq_lens[r]), k)
        start[r], stop[r], keep[r] = st, sp, called == 1
    return start, stop, keep

