"""Independent model of kid_db_read_fragment_votes*: mate pairs called by root-path votes.

numpy only, on top of tests/read_votes_model.py (VoteModel: w, P, best, L, call and the climb) and
tests/read_fragments_model.py (fragment_csr: the CSR of 2 F interleaved reads as a CSR of F fragments).  For one fragment
with mate 1's hit targets a_1 .. a_p, mate 2's b_1 .. b_q and the mates' windows n_1, n_2:

  the multiset  {a_1 .. a_p} + {b_1 .. b_q}, m = p + q, n = (n_1 + n_2) modulo 2^32
  eight fields  the VoteModel record of a read with those m hits and that n
  call_1        the vote call of a_1 .. a_p alone, call_2 that of b_1 .. b_q alone; 0 without a hit

FragmentVoteModel.batch_literal follows the definition per fragment with Python lists; batch_anc is VoteModel's
vectorised form over the fragment CSR, with the per-read calls de-interleaved.  tests/test_read_fragment_votes_model.py
holds the two against each other.  It knows nothing of the library.
"""
import numpy as np

from read_fragments_model import fragment_csr
from read_votes_model import VOTE_DTYPE

FRAGMENT_VOTE_DTYPE = np.dtype([(name, np.uint32) for name in VOTE_DTYPE.names] + [("call_1", np.uint32), ("call_2", np.uint32)])


class FragmentVoteModel:
    def __init__(self, vote_model):
        self.vm = vote_model
        self.sm = vote_model.sm

    def fragment_literal(self, t1, n1, t2, n2, rule):
        """one fragment from the mates' target lists and windows -> the ten fields"""
        t1, t2 = [int(t) for t in t1], [int(t) for t in t2]
        n = (int(n1) + int(n2)) & 0xFFFFFFFF
        return self.vm.read_literal(t1 + t2, n, rule) + (self.vm.call_literal(t1)[0], self.vm.call_literal(t2)[0])

    def batch_literal(self, hits, rule):
        nf = (hits.offsets.size - 1) // 2
        out = np.zeros(nf, FRAGMENT_VOTE_DTYPE)
        for i in range(nf):
            out[i] = self.fragment_literal(hits.of(2 * i)[1].tolist(), hits.n_kmers[2 * i], hits.of(2 * i + 1)[1].tolist(),
                                           hits.n_kmers[2 * i + 1], rule)
        return out

    def batch_anc(self, hits, rule, read_calls=None):
        """read_calls: VoteModel.calls_anc(hits) of the 2 F reads, when the caller has it"""
        v = self.vm.batch_anc(fragment_csr(hits), rule)
        per_read = (self.vm.calls_anc(hits) if read_calls is None else read_calls)[0]
        out = np.zeros(v.size, FRAGMENT_VOTE_DTYPE)
        for f in v.dtype.names:
            out[f] = v[f]
        out["call_1"], out["call_2"] = per_read[0::2], per_read[1::2]
        return out

    def tally(self, hits, rec, counted, entry_targets):
        """SupportModel.tally over the fragments with the vote records' `confident` -> (gcount, ucount)"""
        return self.sm.tally(fragment_csr(hits), rec, counted, entry_targets)


def exchanged(hits):
    """the two mates of every fragment exchanged: reads 2i and 2i + 1 swap places with their hits and n_kmers"""
    from read_hits_model import Hits
    n = hits.offsets.size - 1
    assert n % 2 == 0
    order = np.arange(n).reshape(-1, 2)[:, ::-1].reshape(-1)
    per = np.diff(hits.offsets.astype(np.int64))
    idx = np.concatenate([np.arange(int(hits.offsets[r]), int(hits.offsets[r + 1])) for r in order] + [np.empty(0, np.int64)]).astype(np.int64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(per[order])
    return Hits(off, hits.n_kmers[order], hits.pos[idx], hits.target[idx], hits.entry[idx])


def exchanged_records(rec):
    out = rec.copy()
    out["call_1"], out["call_2"] = rec["call_2"], rec["call_1"]
    return out
