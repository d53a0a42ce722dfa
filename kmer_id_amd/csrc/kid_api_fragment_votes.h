// kid_api_fragment_votes.h -- call mate pairs by root-path votes: kid_db_read_fragment_votes* over the hit pass and the
// two kernels of kid_fragment_votes.hip.h.  The batch is 2 F reads in interleaved order, as for kid_api_fragments.h; the
// family is KidFragmentVoteCalls on the call path of kid_api_support.h (kid_calls_*), with the two-read unit of
// KidFragmentCalls and a hook like that of KidVoteCalls: it binds a scratch set of its own in the database's KidHitsState
// (the list of fragments with more than KID_VOTE_WAVE_HITS hits, its length, one row uint32[ntar] per workgroup of the
// second kernel) and queues kid_fragment_vote_kernel and kid_fragment_vote_big_kernel behind each other between the two
// events of the timer `fragment_votes`.  The set is not the vote family's: a vote call and a fragment-vote call queued
// on two streams touch different lists and rows.  A call waits for the fragment-vote kernels of the call before it
// (KID_SETTLE_FRAGMENT_VOTES) before it binds the set again.  Included behind kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_fragment_votes.hip.h"

static_assert(sizeof(kid_fragment_vote) == sizeof(KidFragmentVote), "kid_fragment_vote is the device record");

struct KidFragmentVoteCalls {
    typedef KidFragmentVote Rec;
    static constexpr uint64_t unit_reads = 2;
    static constexpr unsigned settle = KID_SETTLE_SUPPORT | KID_SETTLE_FRAGMENT_VOTES;
    static constexpr KidDevBuf KidHitsState::*out = &KidHitsState::out_fragment_votes;
    static constexpr KidSpanTimer KidHitsState::*timer = &KidHitsState::fragment_votes;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_fragment_vote_kernel<ROWS, TALLY, DEPTH>; }

    // n: the batch's fragments
    template <bool ROWS, bool TALLY, bool DEPTH>
    static int queue(kid_db *db, KidHitsState *h, dim3 grid, hipStream_t stream, const KidDevDb &d, const uint64_t *d_hit_offsets,
                     const KidHit *d_hits, const uint32_t *d_n_kmers, uint64_t n, KidSupportRule rule, KidFragmentVote *d_out,
                     const KidSupportTally &t)
    {
        const unsigned big_grid = (unsigned)db->num_cu;
        const size_t rows_nbytes = (size_t)big_grid * (size_t)d.ntar * 4u;
        KID_HIP(kid_hits_ensure(h->fvote_list, n * 4u));
        if (!h->fvote_n_list.p) KID_HIP(h->fvote_n_list.alloc(4));
        if (rows_nbytes > h->fvote_rows.cap) { // (the kernels leave it zero)
            KID_HIP(h->fvote_rows.alloc(rows_nbytes));
            KID_HIP(hipMemsetAsync(h->fvote_rows.p, 0, rows_nbytes, stream));
        }
        const KidVoteBig big{h->fvote_list.as<uint32_t>(), h->fvote_n_list.as<uint32_t>(), h->fvote_rows.as<uint32_t>()};
        KID_HIP(hipMemsetAsync(big.n_list, 0, 4, stream));
        hipLaunchKernelGGL((kernel<ROWS, TALLY, DEPTH>()), grid, dim3(256), 0, stream, d, d_hit_offsets, d_hits, d_n_kmers, n, rule, d_out, t, big);
        hipLaunchKernelGGL((kid_fragment_vote_big_kernel<ROWS, TALLY, DEPTH>), dim3(big_grid), dim3(256), 0, stream, d, d_hit_offsets, d_hits,
                           d_n_kmers, n, rule, d_out, t, big);
        return KID_OK;
    }
};

static int kid_fragment_votes_check_args(const kid_db *db, uint64_t n_reads, uint32_t min_permille, const void *out, const kid_sample *tally)
{
    const int rc = kid_calls_check_args<KidFragmentVoteCalls>(db, n_reads, min_permille, tally);
    if (rc != KID_OK) return rc;
    if (n_reads && !out && !tally) return kid_fail(KID_ERR_ARG, "null argument");
    return KID_OK;
}

extern "C" int kid_db_read_fragment_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                          uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally)
{
    int rc = kid_fragment_votes_check_args(db, n_reads, min_permille, out, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, KidFragmentVoteCalls::settle)) != KID_OK) return rc;
    return kid_calls_host_run<KidFragmentVoteCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_read_fragment_votes_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1,
                                                const uint8_t *text2, uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments,
                                                uint32_t min_hits, uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally)
{
    if (n_fragments > 0x3FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^30-1 fragments per batch");
    int rc = kid_fragment_votes_check_args(db, 2 * n_fragments, min_permille, out, tally);
    if (rc != KID_OK || n_fragments == 0) return rc;
    if (!recs1 || !recs2 || (!text1 && nbytes1) || (!text2 && nbytes2)) return kid_fail(KID_ERR_ARG, "null argument");
    // one staged text: the shifted offsets of block 2 are 32-bit like every kid_fastq_rec
    if (nbytes1 + nbytes2 < nbytes1 || nbytes1 + nbytes2 >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "two FASTQ blocks of 4 GiB or more together");
    KidOpenBatch ob;
    rc = kid_hits_open_fastq(ob, db, text1, nbytes1, recs1, 2 * n_fragments, KidFragmentVoteCalls::settle, nullptr, text2, nbytes2, recs2);
    if (rc != KID_OK) return rc;
    return kid_calls_host_run<KidFragmentVoteCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_fragment_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                      uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidFragmentVoteCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_fragment_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, &KidHitsState::fragment_votes, false, device_ms, calls, fragments);
}
