// kid_segment_votes.hip.h -- call segments by root-path votes (kid_db_read_segment_votes*): the vote rule of
// kid_votes.hip.h applied along the record, as kid_segments.hip.h applies the support rule.  The geometry is that file's
// and is computed by its functions alone (kid_segments_of, kid_segments_read_of, kid_segments_before over the two prefix
// arrays the hit pass and the valid scan leave): segment j of a read covers [j * seg_step, min(j * seg_step + seg_len, P)),
// its hits are the contiguous run hits[h0 .. h0 + m) of the read's hit list, its n the valid windows it covers.  Overlapping
// segments share hits: there is no CSR over segments and no copy of the hits per segment, the vote functions take (h, m).
//
//   kid_segment_votes_kernel      64 consecutive segments per wave.  A lane derives (pos, n_pos, h0, m, n_kmers) with the
//                                 four prefix queries, then by m:
//                                   m <= KID_VOTE_LANE_HITS   the lane, kid_vote_lane
//                                   m <= KID_VOTE_WAVE_HITS   the whole wave, the ballot's segments one after the other,
//                                                             kid_vote_wave
//                                   more                      the segment is appended to a device list -- its index, h0, m
//                                                             and n_kmers, 24 bytes -- and nothing is written for it here
//   kid_segment_votes_big_kernel  queued behind it: one workgroup per listed segment over a row uint32[ntar] of scratch
//                                 (kid_vote_big_best / _climb / _clear), the list's length read on the device.  It
//                                 derives pos and n_pos of its segment again (one search, two loads) and writes the
//                                 whole record: every output word has one writer.
// The caps are those of kid_segments_kernel: a batch with more hits than hits_cap or more segments than seg_cap is left
// alone by both kernels (the first appends nothing then; the second tests the same condition, so a stale list length
// cannot reach it either).  The list's order is not deterministic; nothing read from it depends on that.  Pure, integer,
// no atomics on outputs: byte-identical across runs, across splits of the reads into calls and across table kinds.
//
// Cost: the lane regime is O(m^2) <= 64 pair tests per segment, the wave regime O(m^2 / 64) <= 4096 steps per lane, the
// workgroup regime O(m * depth) row accesses.  Under overlap a hit is visited once per segment that covers it, up to
// KID_SEGMENT_MAX_OVERLAP times: that is the rule's cost (a sliding row would remove it and is not built).
#pragma once
#include "kid_segments.hip.h"
#include "kid_votes.hip.h"

struct KidSegmentVote { // = kid_segment_vote (include/kmer_id_amd.h)
    uint32_t pos, n_pos;
    KidVote v;
};

struct KidSegmentVoteEntry { // a segment left to kid_segment_votes_big_kernel
    uint64_t seg, h0;
    uint32_t m, n_kmers;
};
struct KidSegmentVoteBig {
    KidSegmentVoteEntry *list; // as many as the call can write segments
    uint32_t *n_list;          // their number: zeroed in front of kid_segment_votes_kernel
    uint32_t *rows;            // one row uint32[ntar] per workgroup of kid_segment_votes_big_kernel, zero between segments
    uint64_t list_cap;
};

template <bool ROWS>
__global__ __launch_bounds__(256) void kid_segment_votes_kernel(const KidDevDb db, const KidSegmentsIn a, const KidSegGeom g,
                                                                 const KidSupportRule rule, KidSegmentVote *out, const KidSegmentVoteBig big)
{
    kid_calls_run<false, false>(KidSegmentUnits<KidSegmentVote, KidSegmentVoteBig>{a, g, a.hits, out, big}, KidVoteMethod<ROWS>{db, rule},
                                KidSupportTally());
}

// ------------------------------------------------------------------ segments of more than KID_VOTE_WAVE_HITS hits
template <bool ROWS>
__global__ __launch_bounds__(256) void kid_segment_votes_big_kernel(const KidDevDb db, const KidSegmentsIn a, const KidSegGeom g,
                                                                     const KidSupportRule rule, KidSegmentVote *out, const KidSegmentVoteBig big)
{
    __shared__ uint32_t sh[4 * 9]; // as in kid_vote_big_kernel
    const uint64_t n_seg = a.seg_offsets[a.n_reads];
    if (!kid_segments_fits(a, n_seg)) return;
    uint32_t *row = big.rows + (uint64_t)blockIdx.x * (uint64_t)db.ntar;
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list && e < big.list_cap; e += gridDim.x) {
        const KidSegmentVoteEntry en = big.list[e];
        const KidHit *h = a.hits + en.h0;
        KidSegmentVote res = {0u, 0u, {0u, 0u, en.n_kmers, en.m, 0u, 0u, 0u, 0u}};
        uint32_t best, nb, call;
        uint4 cr;
        kid_vote_big_best<ROWS>(db, row, h, en.m, sh, best, nb, call, cr);
        res.v.p_best = best;
        res.v.n_best = nb;
        kid_vote_big_climb<ROWS>(db, h, en.m, sh, call, cr, rule, res.v);
        if (threadIdx.x == 0) {
            const uint64_t r = kid_segments_read_of(a.seg_offsets, 0, a.n_reads, en.seg);
            uint64_t q_lo, q_hi;
            kid_segments_place(a, g, r, en.seg, a.desc[r], q_lo, q_hi, res.pos, res.n_pos);
            out[en.seg] = res;
        }
        kid_vote_big_clear(db, row, h, en.m);
    }
}
