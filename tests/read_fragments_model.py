"""Independent model of kid_db_read_fragments*: mate pairs called as one fragment.

numpy and the oracle binding only, on top of tests/read_hits_model.py and tests/read_support_model.py: HitModel.batch gives
the hits of the 2 F reads (interleaved: read 2i = mate 1 of fragment i, read 2i + 1 = its mate 2), HitModel.fold the folds,
SupportModel.read_literal the six support fields.  For one fragment with mate 1's hit targets a_1 .. a_p, mate 2's
b_1 .. b_q and the mates' windows n_1, n_2:

  the sequence  a_1 .. a_p, b_1 .. b_q (concatenated lists), n = n_1 + n_2
  six fields    SupportModel.read_literal(sequence, n, rule, fold(sequence))
  final_1       fold(a), final_2 = fold(b); 0 without a hit

It knows nothing of the library.
"""
import numpy as np

from read_hits_model import Hits

FRAGMENT_DTYPE = np.dtype([("final", np.uint32), ("confident", np.uint32), ("n_kmers", np.uint32), ("n_hits", np.uint32),
                           ("s_final", np.uint32), ("s_confident", np.uint32), ("final_1", np.uint32), ("final_2", np.uint32)])


def fragment_csr(hits):
    """the CSR of 2 F reads as a CSR of F fragments: every other offset, n_kmers added up per pair"""
    assert (hits.offsets.size - 1) % 2 == 0
    nk = hits.n_kmers.astype(np.int64)
    return Hits(hits.offsets[::2].copy(), (nk[0::2] + nk[1::2]).astype(np.uint32), hits.pos, hits.target, hits.entry)


class FragmentModel:
    def __init__(self, support_model):
        self.sm = support_model
        self.hm = support_model.hm

    def fragment(self, t1, n1, t2, n2, rule):
        """one fragment from the mates' target lists and windows -> the eight fields"""
        seq = list(t1) + list(t2)
        final = self.hm.fold(seq)
        return self.sm.read_literal(seq, int(n1) + int(n2), rule, final) + (self.hm.fold(t1), self.hm.fold(t2))

    def batch(self, hits, rule):
        nf = (hits.offsets.size - 1) // 2
        out = np.zeros(nf, FRAGMENT_DTYPE)
        for i in range(nf):
            out[i] = self.fragment(hits.of(2 * i)[1].tolist(), hits.n_kmers[2 * i], hits.of(2 * i + 1)[1].tolist(), hits.n_kmers[2 * i + 1], rule)
        return out

    def tally(self, hits, rec, counted, entry_targets):
        """SupportModel.tally over the fragments: gcount[confident]++ per counted fragment; the entries of the hits with
        target > 1 of both mates of counted fragments with confident > 0 are seen -> (gcount, ucount)"""
        return self.sm.tally(fragment_csr(hits), rec, counted, entry_targets)


def interleave(seqs1, seqs2):
    """[mate 1 of fragment 0, mate 2 of fragment 0, mate 1 of fragment 1, ..]"""
    assert len(seqs1) == len(seqs2)
    return [s for pair in zip(seqs1, seqs2) for s in pair]
