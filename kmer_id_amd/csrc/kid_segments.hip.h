// kid_segments.hip.h -- call records in segments (kid_db_read_segments*): kid_support.hip.h applied along the record.
// A read with P window positions (its descriptor's n_kmers) is cut into segments of seg_len positions, seg_step apart:
//   n_seg = 0 (P = 0), 1 (P <= seg_len), else 1 + ceil((P - seg_len) / seg_step)
//   segment j covers the positions [j * seg_step, min(j * seg_step + seg_len, P))
// and each segment is called by ITS hits under the support rule: the kid_support record of the read cut to the segment.
//
// Input: what the hit pass leaves behind (kid_hits.hip.h): the descriptors, the first tile of every read, per tile of 64
// positions the mask of its hit lanes and -- asked for by KidHitsTiles::tile_valid -- the mask of its lanes that hold a
// k-mer, the exclusive scan of the hit masks' popcounts (= where a tile's hits start in the hit array) and the hits.
// With a second scan, over the valid masks, the hits and the valid windows in front of position x of read r are
//   prefix[tile_off[r] + x / 64] + popc(mask[that tile] & low(x % 64))
// (kid_segments_before: the mask is not loaded when x % 64 == 0 -- the tile index may then be the first tile of the next
// read or the batch's tile count, which the prefix arrays have and the mask arrays do not).  A segment's n_kmers and its
// hit range [h_lo, h_hi) are two such queries each: O(1) whatever its length, no search over pos.
//
//   kid_segments_count_kernel   segments per read, from its descriptor
//   kid_hits_scan_*<2>          -> seg_offsets[n_reads + 1] (in place)
//   kid_hits_scan_*<1>          popcount(valid mask) per tile -> valid windows in front of every tile
//   kid_segments_kernel         kid_calls_run (kid_calls.hip.h) over KidSegmentUnits with the support kernel's method
// Pure, integer, no atomics, every output place a function of the batch: byte-identical across runs, across splits of
// the reads into calls and across table kinds.
#pragma once
#include "kid_hits.hip.h"
#include "kid_support.hip.h"

struct KidSegment { // = kid_segment (include/kmer_id_amd.h)
    uint32_t pos, n_pos;
    KidSupport s;
};

struct KidSegGeom {
    uint32_t seg_len, seg_step;
};

// segments of a read of P positions
__device__ __forceinline__ uint64_t kid_segments_of(uint64_t P, const KidSegGeom &g)
{
    if (P == 0) return 0ull;
    if (P <= g.seg_len) return 1ull;
    return 1ull + (P - g.seg_len + g.seg_step - 1u) / g.seg_step;
}

// n_seg[r] per read.  A batch whose tiles did not fit its scratch (tile_off[n_reads] == 0: kid_hits_scan_top_kernel) has
// no tile, no hit and no segment.
__global__ void kid_segments_count_kernel(const KidReadDesc *desc, const uint64_t *tile_off, uint64_t n_reads, const KidSegGeom g,
                                          uint64_t *n_seg)
{
    const bool tiles = tile_off[n_reads] != 0;
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const int32_t nk = desc[r].n_kmers;
        n_seg[r] = tiles && nk > 0 ? kid_segments_of((uint64_t)(uint32_t)nk, g) : 0ull;
    }
}

struct KidSegmentsIn {
    const KidReadDesc *desc;
    const uint64_t *tile_off;      // [n_reads + 1]
    const uint64_t *seg_offsets;   // [n_reads + 1]
    uint64_t n_reads;
    const unsigned long long *tile_mask, *tile_valid; // [tiles]
    const uint64_t *tile_hit_off, *tile_valid_off;    // [tiles + 1]
    const KidHit *hits;
    const uint64_t *offsets;       // read origins, or
    const KidFastqRec *recs;
    uint64_t hits_cap, seg_cap;    // nothing is written when the batch has more hits, or more segments, than these
};

// bits of the tiles' masks in front of position x of the read whose first tile is t0
__device__ __forceinline__ uint64_t kid_segments_before(const uint64_t *prefix, const unsigned long long *mask, uint64_t t0, uint64_t x)
{
    const uint64_t t = t0 + x / KID_HITS_TILE;
    const uint32_t low = (uint32_t)(x % KID_HITS_TILE);
    uint64_t v = prefix[t];
    if (low) v += (uint64_t)__popcll(mask[t] & ((1ull << low) - 1ull));
    return v;
}

// the read of segment s among the reads [lo, hi): seg_offsets[lo] <= s < seg_offsets[hi] (reads without a segment own none)
__device__ __forceinline__ uint64_t kid_segments_read_of(const uint64_t *seg_offsets, uint64_t lo, uint64_t hi, uint64_t s)
{
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (seg_offsets[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// pos and n_pos of segment s of read r (descriptor d), and the positions [q_lo, q_hi) of the read it covers
__device__ __forceinline__ void kid_segments_place(const KidSegmentsIn &a, const KidSegGeom &g, uint64_t r, uint64_t s, const KidReadDesc &d,
                                                   uint64_t &q_lo, uint64_t &q_hi, uint32_t &pos, uint32_t &n_pos)
{
    const uint64_t P = (uint64_t)(uint32_t)d.n_kmers;
    q_lo = (s - a.seg_offsets[r]) * g.seg_step;
    q_hi = P - q_lo > g.seg_len ? q_lo + g.seg_len : P;
    const uint64_t origin = a.offsets ? a.offsets[r] : (uint64_t)a.recs[r].seq_off;
    pos = (uint32_t)(d.first_base - origin + q_lo);
    n_pos = (uint32_t)(q_hi - q_lo);
}

__device__ __forceinline__ bool kid_segments_fits(const KidSegmentsIn &a, uint64_t n_seg)
{
    return n_seg <= a.seg_cap && a.tile_hit_off[a.tile_off[a.n_reads]] <= a.hits_cap;
}

// the segments of a batch as the units of kid_calls_run: Out is {pos, n_pos, the method's record}.  Big: the list of the
// family's second kernel ({list, n_list, list_cap}: entries of {segment, h0, m, n_kmers}), or nothing
struct KidNoList {};
template <class Out, class Big>
struct KidSegmentUnits {
    const KidSegmentsIn &a;
    const KidSegGeom &g;
    const KidHit *hits;
    Out *out;
    Big big;
    struct Unit {
        uint64_t h0;
        uint32_t m, n_kmers, pos, n_pos;
    };
    struct Span {
        uint64_t r_first, r_last;
    };
    __device__ __forceinline__ uint64_t count() const
    {
        const uint64_t n_seg = a.seg_offsets[a.n_reads];
        return kid_segments_fits(a, n_seg) ? n_seg : 0ull;
    }
    // the reads of the wave's first and last segment (wave-uniform searches), then every lane's own between them:
    // 64 segments of a metagenomic batch are 64 reads, six steps; reads without a window in between cost nothing
    __device__ __forceinline__ Span span(uint64_t s0, uint64_t n_seg) const
    {
        const uint64_t s_last = n_seg - s0 > 64u ? s0 + 63u : n_seg - 1u;
        const uint64_t r_first = kid_segments_read_of(a.seg_offsets, 0, a.n_reads, s0);
        return Span{r_first, kid_segments_read_of(a.seg_offsets, r_first, a.n_reads, s_last)};
    }
    __device__ __forceinline__ void find(const Span &sp, uint64_t s, Unit &un) const
    {
        const uint64_t r = kid_segments_read_of(a.seg_offsets, sp.r_first, sp.r_last + 1u, s);
        const uint64_t t0 = a.tile_off[r];
        uint64_t q_lo, q_hi;
        kid_segments_place(a, g, r, s, a.desc[r], q_lo, q_hi, un.pos, un.n_pos);
        un.h0 = kid_segments_before(a.tile_hit_off, a.tile_mask, t0, q_lo);
        un.m = (uint32_t)(kid_segments_before(a.tile_hit_off, a.tile_mask, t0, q_hi) - un.h0);
        un.n_kmers = (uint32_t)(kid_segments_before(a.tile_valid_off, a.tile_valid, t0, q_hi) -
                                kid_segments_before(a.tile_valid_off, a.tile_valid, t0, q_lo));
    }
    __device__ __forceinline__ void append(uint64_t s, const Unit &un) const
    {
        const uint32_t e = atomicAdd(big.n_list, 1u);
        if (e < big.list_cap) big.list[e] = {s, un.h0, un.m, un.n_kmers};
    }
    template <class R>
    __device__ __forceinline__ void store(uint64_t s, const Unit &un, const R &res) const
    {
        out[s] = Out{un.pos, un.n_pos, res};
    }
};

template <bool ROWS>
__global__ __launch_bounds__(256) void kid_segments_kernel(const KidDevDb db, const KidSegmentsIn a, const KidSegGeom g, const KidSupportRule rule,
                                                            KidSegment *out)
{
    kid_calls_run<false, false>(KidSegmentUnits<KidSegment, KidNoList>{a, g, a.hits, out, KidNoList()}, KidSupportMethod<ROWS>{db, rule},
                                KidSupportTally());
}
