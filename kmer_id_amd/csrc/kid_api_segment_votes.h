// kid_api_segment_votes.h -- call segments by root-path votes: kid_db_read_segment_votes* over the hit pass, the scans of
// kid_api_segments.h (kid_segments_size, KidWantValid, kid_segments_launch_scans: the geometry is computed once, there)
// and the two kernels of kid_segment_votes.hip.h.  The family is KidSegmentVoteCalls on the three forms of
// kid_api_segments.h (kid_segment_calls_*), so the quartet is kid_db_read_segments* argument for argument, check for
// check; its launch binds the scratch and queues the two kernels behind each other.  The kernels run between the two
// events of the family's timer; like the segment kernels they read the tiles' scratch behind the pass, so every
// later call on the database waits for them (KID_SETTLE_ALWAYS).  The scratch is KidHitsState::segment_vote_big:
// the list of segments with more than KID_VOTE_WAVE_HITS hits (24 B per segment the call can write: the host forms know
// the total, the device form has seg_cap) and its length are the family's own; the rows are the vote family's
// (vote_big.own_rows) -- a call settles the support and vote timers before it binds them, and a vote call waits
// for this family's timer as every call does.  Included behind kid_api_segments.h and kid_api_votes.h.
#pragma once
#include "kid_api_segments.h"
#include "kid_api_votes.h"
#include "kid_segment_votes.hip.h"

static_assert(sizeof(kid_segment_vote) == sizeof(KidSegmentVote) && sizeof(KidSegmentVote) == 40, "kid_segment_vote is the device record");

struct KidSegmentVoteCalls {
    typedef KidSegmentVote Rec;
    static constexpr KidFamily id = KID_FAM_SEGMENT_VOTES;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT) | kid_settle(KID_FAM_VOTES);
    // a.seg_cap: the segments the call can write, which the list is sized for
    static int launch(kid_db *db, KidHitsState *h, const KidSegmentsIn &a, KidSegGeom g, KidSupportRule rule, KidSegmentVote *d_segments,
                      hipStream_t stream)
    {
        KidVoteScratch &s = h->segment_vote_big;
        const int rc = kid_vote_scratch_bind(db, s, a.seg_cap * sizeof(KidSegmentVoteEntry), stream);
        if (rc != KID_OK) return rc;
        const KidSegmentVoteBig big{s.list.as<KidSegmentVoteEntry>(), s.n_list.as<uint32_t>(), s.rows->as<uint32_t>(), a.seg_cap};
        const dim3 grid(kid_grid_for(a.seg_cap, 256, db->num_cu * 8)), block(256);
        kid_lift(db->d.rows != nullptr, [&](auto rows) {
            hipLaunchKernelGGL((kid_segment_votes_kernel<decltype(rows)::value>), grid, block, 0, stream, db->d, a, g, rule, d_segments, big);
            hipLaunchKernelGGL((kid_segment_votes_big_kernel<decltype(rows)::value>), dim3(db->num_cu), block, 0, stream, db->d, a, g, rule,
                               d_segments, big);
        });
        return KID_OK;
    }
};

extern "C" int kid_db_read_segment_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                         uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                                         uint64_t *seg_offsets, kid_segment_vote *segments, uint64_t cap, uint64_t *n_segments)
{
    return kid_segment_calls_offsets<KidSegmentVoteCalls>(db, bases, offsets, start, stop, n_reads, seg_len, seg_step, min_hits, min_permille,
                                                          seg_offsets, segments, cap, n_segments);
}

extern "C" int kid_db_read_segment_votes_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                               uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                                               uint64_t *seg_offsets, kid_segment_vote *segments, uint64_t cap, uint64_t *n_segments)
{
    return kid_segment_calls_fastq<KidSegmentVoteCalls>(db, text, text_nbytes, recs, n_reads, seg_len, seg_step, min_hits, min_permille,
                                                        seg_offsets, segments, cap, n_segments);
}

extern "C" int kid_db_read_segment_votes_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                                const void *d_stop, uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits,
                                                uint32_t min_permille, void *d_hits, uint64_t hits_cap, void *d_seg_offsets, void *d_segments,
                                                uint64_t seg_cap, void *d_n_hits, void *d_n_segments, void *stream)
{
    return kid_segment_calls_device<KidSegmentVoteCalls>(db, d_bases, bases_nbytes, d_offsets, d_start, d_stop, n_reads, seg_len, seg_step,
                                                         min_hits, min_permille, d_hits, hits_cap, d_seg_offsets, d_segments, seg_cap, d_n_hits,
                                                         d_n_segments, stream);
}

extern "C" int kid_db_read_segment_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KidSegmentVoteCalls::id, device_ms, calls, reads);
}
