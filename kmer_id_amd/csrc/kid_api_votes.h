// kid_api_votes.h -- call reads by root-path votes: kid_db_read_votes* over the hit pass and the two kernels of
// kid_votes.hip.h.  The family is KidVoteCalls on the call path of kid_api_support.h (kid_calls_*: checks, host run,
// tally binding, the four forms); kid_calls_queue binds its KidVoteScratch in the database's KidHitsState (vote_big:
// the list of reads with more than KID_VOTE_WAVE_HITS hits, its length, one row uint32[ntar] per workgroup of the second
// kernel) and queues kid_vote_kernel and kid_vote_big_kernel behind each other between the two events of the family's
// timer.  The scratch grows with the largest batch and with num_cu * ntar, never with the table; a call waits for the
// vote kernels of the call before it (kid_settle(KID_FAM_VOTES)) before it binds the scratch again.  Included behind
// kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_votes.hip.h"

static_assert(sizeof(kid_vote) == sizeof(KidVote), "kid_vote is the device record");

struct KidVoteCalls {
    typedef KidVote Rec;
    static constexpr KidFamily id = KID_FAM_VOTES;
    static constexpr uint64_t unit_reads = 1;
    static constexpr bool needs_sink = false;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT) | kid_settle(KID_FAM_VOTES);
    static constexpr KidVoteScratch KidHitsState::*big = &KidHitsState::vote_big;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_vote_kernel<ROWS, TALLY, DEPTH>; }
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto big_kernel() { return &kid_vote_big_kernel<ROWS, TALLY, DEPTH>; }
};

extern "C" int kid_db_read_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                 uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally)
{
    return kid_calls_offsets<KidVoteCalls>(db, bases, offsets, start, stop, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_read_votes_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                       uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally)
{
    return kid_calls_fastq<KidVoteCalls>(db, text, text_nbytes, recs, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                             uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidVoteCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KidVoteCalls::id, device_ms, calls, reads);
}
