// kid_api_fragment_votes.h -- call mate pairs by root-path votes: kid_db_read_fragment_votes* over the hit pass and the
// two kernels of kid_fragment_votes.hip.h.  The batch is 2 F reads in interleaved order, as for kid_api_fragments.h; the
// family is KidFragmentVoteCalls on the call path of kid_api_support.h (kid_calls_*), with the two-read unit of
// KidFragmentCalls and a second kernel like KidVoteCalls: kid_calls_queue binds a KidVoteScratch of its own in the
// database's KidHitsState (fragment_vote_big: the list of fragments with more than KID_VOTE_WAVE_HITS hits, its length,
// one row uint32[ntar] per workgroup of the second kernel) and queues kid_fragment_vote_kernel and
// kid_fragment_vote_big_kernel behind each other between the two events of the family's timer.  The set is not the vote
// family's: a vote call and a fragment-vote call queued on two streams touch different lists and rows.  A call waits
// for the fragment-vote kernels of the call before it (kid_settle(KID_FAM_FRAGMENT_VOTES)) before it binds the set
// again.  Included behind kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_fragment_votes.hip.h"

static_assert(sizeof(kid_fragment_vote) == sizeof(KidFragmentVote), "kid_fragment_vote is the device record");

struct KidFragmentVoteCalls {
    typedef KidFragmentVote Rec;
    static constexpr KidFamily id = KID_FAM_FRAGMENT_VOTES;
    static constexpr uint64_t unit_reads = 2;
    static constexpr bool needs_sink = true;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT) | kid_settle(KID_FAM_FRAGMENT_VOTES);
    static constexpr KidVoteScratch KidHitsState::*big = &KidHitsState::fragment_vote_big;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_fragment_vote_kernel<ROWS, TALLY, DEPTH>; }
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto big_kernel() { return &kid_fragment_vote_big_kernel<ROWS, TALLY, DEPTH>; }
};

extern "C" int kid_db_read_fragment_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                          uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally)
{
    return kid_calls_offsets<KidFragmentVoteCalls>(db, bases, offsets, start, stop, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_read_fragment_votes_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1,
                                                const uint8_t *text2, uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments,
                                                uint32_t min_hits, uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally)
{
    return kid_calls_fastq_pairs<KidFragmentVoteCalls>(db, text1, nbytes1, recs1, text2, nbytes2, recs2, n_fragments, min_hits, min_permille,
                                                       out, tally);
}

extern "C" int kid_db_fragment_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                      uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidFragmentVoteCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_fragment_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, KidFragmentVoteCalls::id, device_ms, calls, fragments);
}
