// kid_api_votes.h -- call reads by root-path votes: kid_db_read_votes* over the hit pass and the two kernels of
// kid_votes.hip.h.  The family is KidVoteCalls on the call path of kid_api_support.h (kid_calls_*: checks, host run,
// tally binding, device form); its hook (kid_calls_queue) binds the scratch of the database's KidHitsState -- the list
// of reads with more than KID_VOTE_WAVE_HITS hits, its length, one row uint32[ntar] per workgroup of the second kernel --
// and queues kid_vote_kernel and kid_vote_big_kernel behind each other between the two events of the timer `votes`: the
// second reads the list's length on the device, there is no host round trip.  The scratch grows with the largest batch
// and with num_cu * ntar, never with the table; a call waits for the vote kernels of the call before it
// (KID_SETTLE_VOTES) before it binds the scratch again.  Included behind kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_votes.hip.h"

static_assert(sizeof(kid_vote) == sizeof(KidVote), "kid_vote is the device record");

struct KidVoteCalls {
    typedef KidVote Rec;
    static constexpr uint64_t unit_reads = 1;
    static constexpr unsigned settle = KID_SETTLE_SUPPORT | KID_SETTLE_VOTES;
    static constexpr KidDevBuf KidHitsState::*out = &KidHitsState::out_votes;
    static constexpr KidSpanTimer KidHitsState::*timer = &KidHitsState::votes;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_vote_kernel<ROWS, TALLY, DEPTH>; }

    template <bool ROWS, bool TALLY, bool DEPTH>
    static int queue(kid_db *db, KidHitsState *h, dim3 grid, hipStream_t stream, const KidDevDb &d, const uint64_t *d_hit_offsets,
                     const KidHit *d_hits, const uint32_t *d_n_kmers, uint64_t n, KidSupportRule rule, KidVote *d_out, const KidSupportTally &t)
    {
        const unsigned big_grid = (unsigned)db->num_cu;
        const size_t rows_nbytes = (size_t)big_grid * (size_t)d.ntar * 4u;
        KID_HIP(kid_hits_ensure(h->vote_list, n * 4u));
        if (!h->vote_n_list.p) KID_HIP(h->vote_n_list.alloc(4));
        if (rows_nbytes > h->vote_rows.cap) { // (the kernels leave it zero)
            KID_HIP(h->vote_rows.alloc(rows_nbytes));
            KID_HIP(hipMemsetAsync(h->vote_rows.p, 0, rows_nbytes, stream));
        }
        const KidVoteBig big{h->vote_list.as<uint32_t>(), h->vote_n_list.as<uint32_t>(), h->vote_rows.as<uint32_t>()};
        KID_HIP(hipMemsetAsync(big.n_list, 0, 4, stream));
        hipLaunchKernelGGL((kernel<ROWS, TALLY, DEPTH>()), grid, dim3(256), 0, stream, d, d_hit_offsets, d_hits, d_n_kmers, n, rule, d_out, t, big);
        hipLaunchKernelGGL((kid_vote_big_kernel<ROWS, TALLY, DEPTH>), dim3(big_grid), dim3(256), 0, stream, d, d_hit_offsets, d_hits, d_n_kmers, n,
                           rule, d_out, t, big);
        return KID_OK;
    }
};

extern "C" int kid_db_read_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                 uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally)
{
    int rc = kid_calls_check_args<KidVoteCalls>(db, n_reads, min_permille, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, KidVoteCalls::settle)) != KID_OK) return rc;
    return kid_calls_host_run<KidVoteCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_read_votes_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                       uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally)
{
    int rc = kid_calls_check_args<KidVoteCalls>(db, n_reads, min_permille, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, KidVoteCalls::settle)) != KID_OK) return rc;
    return kid_calls_host_run<KidVoteCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                             uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidVoteCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, &KidHitsState::votes, false, device_ms, calls, reads);
}
