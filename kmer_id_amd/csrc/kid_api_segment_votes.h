// kid_api_segment_votes.h -- call segments by root-path votes: kid_db_read_segment_votes* over the hit pass, the scans of
// kid_api_segments.h (kid_segments_size, KidWantValid, kid_segments_launch_scans: the geometry is computed once, there)
// and the two kernels of kid_segment_votes.hip.h.  The family is KidSegmentVoteCalls on the three forms of
// kid_api_segments.h (kid_segment_calls_*), so the quartet is kid_db_read_segments* argument for argument, check for
// check; its launch binds the scratch and queues the two kernels behind each other.  The kernels run between the two
// events of the timer `segment_votes`; like the segment kernels they read the tiles' scratch behind the pass, so every
// later call on the database waits for them (kid_hits_state).  The scratch:
// the list of segments with more than KID_VOTE_WAVE_HITS hits (24 B per segment the call can write: the host forms know
// the total, the device form has seg_cap) and its length are the family's own; the rows are KidHitsState::vote_rows,
// the vote family's -- a call settles KID_SETTLE_SUPPORT | KID_SETTLE_VOTES before it binds them, and a vote call waits
// for this family's timer as every call does.  Included behind kid_api_segments.h and kid_api_votes.h.
#pragma once
#include "kid_api_segments.h"
#include "kid_api_votes.h"
#include "kid_segment_votes.hip.h"

static_assert(sizeof(kid_segment_vote) == sizeof(KidSegmentVote) && sizeof(KidSegmentVote) == 40, "kid_segment_vote is the device record");

struct KidSegmentVoteCalls {
    typedef KidSegmentVote Rec;
    static constexpr unsigned settle = KID_SETTLE_SUPPORT | KID_SETTLE_VOTES;
    static constexpr KidDevBuf KidHitsState::*out = &KidHitsState::out_segment_votes;
    static constexpr KidSpanTimer KidHitsState::*timer = &KidHitsState::segment_votes;
    // a.seg_cap: the segments the call can write, which the list is sized for
    static int launch(kid_db *db, KidHitsState *h, const KidSegmentsIn &a, KidSegGeom g, KidSupportRule rule, KidSegmentVote *d_segments,
                      hipStream_t stream)
    {
        const unsigned big_grid = (unsigned)db->num_cu;
        const size_t rows_nbytes = (size_t)big_grid * (size_t)db->d.ntar * 4u;
        KID_HIP(kid_hits_ensure(h->svote_list, a.seg_cap * sizeof(KidSegmentVoteEntry)));
        if (!h->svote_n_list.p) KID_HIP(h->svote_n_list.alloc(4));
        if (rows_nbytes > h->vote_rows.cap) { // (the kernels leave it zero)
            KID_HIP(h->vote_rows.alloc(rows_nbytes));
            KID_HIP(hipMemsetAsync(h->vote_rows.p, 0, rows_nbytes, stream));
        }
        const KidSegmentVoteBig big{h->svote_list.as<KidSegmentVoteEntry>(), h->svote_n_list.as<uint32_t>(), h->vote_rows.as<uint32_t>(), a.seg_cap};
        KID_HIP(hipMemsetAsync(big.n_list, 0, 4, stream));
        const dim3 grid(kid_grid_for(a.seg_cap, 256, db->num_cu * 8)), block(256);
        kid_lift(db->d.rows != nullptr, [&](auto rows) {
            hipLaunchKernelGGL((kid_segment_votes_kernel<decltype(rows)::value>), grid, block, 0, stream, db->d, a, g, rule, d_segments, big);
            hipLaunchKernelGGL((kid_segment_votes_big_kernel<decltype(rows)::value>), dim3(big_grid), block, 0, stream, db->d, a, g, rule,
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
    return kid_hits_take_time(db, &KidHitsState::segment_votes, false, device_ms, calls, reads);
}
