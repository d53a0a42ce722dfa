// kid_coverage.hip.h -- breadth of coverage per organism from seen-bitmaps (the layout of kid_sample_seen_export) and the
// two site columns of the probes file: per entry o its organism org[o] and its position pos[o].  With bin(o) = pos[o] / W
//   span_bins[g] = 1 + max bin(o) over the entries of g (0 without one),   bin_base = the exclusive scan of span_bins,
//   probes[bin_base[g] + b] = #{ o : org[o] == g, bin(o) == b },   seen_i[...] = those of them whose bit is set in bitmap i
// and per (bitmap, organism) one kid_coverage record folded from the organism's bins (include/kmer_id_amd.h has the rule).
// Three stages:
//   span    kid_cov_span_kernel (atomicMax of bin + 1 per organism), kid_cov_scan_kernel (one workgroup: bin_base, B)
//   count   kid_cov_count_kernel<ALL>: a workgroup takes a contiguous span of tiles of 64 entries, a wave one tile at a
//           time.  A tile without a bit is skipped: its org and pos are not read.  The lanes of a tile whose global bin is
//           that of the lane before them form a run: a ballot finds the heads, the popcount of the tile's bits inside the
//           run is its sum, and the head issues one atomicAdd.  Runs are an optimisation only: any order of entries is
//           counted right (a run may be one entry long).  ALL = true counts every entry: that is `probes`.
//   reduce  kid_cov_reduce_kernel: one wave per organism walks its bins 64 at a time.
// Counters are 32-bit in global memory throughout; nothing is staged in narrower ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KID_COV_TILE 64u      // entries per tile: one wave, two words of the bitmap
#define KID_COV_MIN_SPAN 16u  // tiles a workgroup takes at least

// The device form of kid_coverage (include/kmer_id_amd.h): eight uint32
struct KidCoverageRec {
    uint32_t n_probes, n_seen, span_bins, bins, bins_seen, max_gap, max_bin_seen, max_bin;
};

__device__ __forceinline__ uint32_t kid_cov_wave_max(uint32_t v)
{
    for (int w = 32; w > 0; w >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, w);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t kid_cov_wave_sum(uint32_t v)
{
    for (int w = 32; w > 0; w >>= 1) v += (uint32_t)__shfl_xor((int)v, w);
    return v;
}
// the bits [lo, hi) of a 64-bit mask (lo <= hi <= 64)
__device__ __forceinline__ uint64_t kid_cov_bits(uint32_t lo, uint32_t hi)
{
    const uint64_t upto_hi = hi >= 64u ? ~0ull : (1ull << hi) - 1ull;
    const uint64_t upto_lo = lo >= 64u ? ~0ull : (1ull << lo) - 1ull;
    return upto_hi & ~upto_lo;
}

// span[g] = max over the entries of g of bin + 1 (saturating: a span of 2^32 is beyond every cap anyway).  The entries of
// a wave that all belong to one organism -- the rule in a file in (org, position) order -- issue one atomicMax.
__global__ __launch_bounds__(256) void kid_cov_span_kernel(const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs,
                                                           uint32_t bin_width, uint32_t *span)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n_entries + stride - 1) / stride; // (the same in every lane: no lane leaves before a shuffle)
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t o = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t g = ~0u, v = 0;
        if (o < n_entries) {
            g = org[o];
            const uint32_t b = pos[o] / bin_width;
            v = b == ~0u ? ~0u : b + 1u;
        }
        const bool valid = g < n_orgs; // (the host has checked the organisms: this keeps a write inside `span` whatever it is given)
        const uint64_t act = __ballot(valid);
        if (!act) continue;
        const uint32_t g0 = (uint32_t)__shfl((int)g, (int)__builtin_ctzll(act));
        if (__ballot(valid && g != g0) == 0) {
            const uint32_t m = kid_cov_wave_max(valid ? v : 0u);
            if ((threadIdx.x & 63u) == 0) atomicMax(&span[g0], m);
        } else if (valid) {
            atomicMax(&span[g], v);
        }
    }
}

// bin_base[g] = span[0] + ... + span[g - 1] for g in 0..n_orgs (64-bit: the sum is checked against the cap by the host)
__global__ __launch_bounds__(256) void kid_cov_scan_kernel(const uint32_t *span, uint32_t n_orgs, unsigned long long *bin_base)
{
    __shared__ unsigned long long part[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = ((uint64_t)n_orgs + 255u) / 256u;
    const uint64_t g0 = per * tid < n_orgs ? per * tid : n_orgs, g1 = g0 + per < n_orgs ? g0 + per : n_orgs;
    unsigned long long sum = 0;
    for (uint64_t g = g0; g < g1; g++) sum += span[g];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (uint32_t t = 0; t < 256u; t++) {
            const unsigned long long s = part[t];
            part[t] = run;
            run += s;
        }
        bin_base[n_orgs] = run;
    }
    __syncthreads();
    unsigned long long run = part[tid];
    for (uint64_t g = g0; g < g1; g++) {
        bin_base[g] = run;
        run += span[g];
    }
}

// counts[bin_base[org[o]] + pos[o] / W] += 1 for every entry o < n_entries whose bit is set (ALL: for every entry).
// n_bins: the size of `counts` (an entry whose bin would fall outside it is not counted: it cannot happen with the
// bin_base of these entries).  span: tiles per workgroup.
template <bool ALL>
__global__ __launch_bounds__(256) void kid_cov_count_kernel(const unsigned long long *bitmap, const uint32_t *org, const uint32_t *pos,
                                                            uint64_t n_entries, uint32_t n_orgs, uint32_t bin_width,
                                                            const unsigned long long *bin_base, uint64_t n_bins, uint64_t n_tiles,
                                                            uint64_t span, uint32_t *counts)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile_begin = (uint64_t)blockIdx.x * span;
    const uint64_t tile_end = tile_begin + span < n_tiles ? tile_begin + span : n_tiles;
    for (uint64_t tile = tile_begin + wave; tile < tile_end; tile += 4u) {
        const uint64_t o0 = tile * KID_COV_TILE;
        const uint64_t in_range = n_entries - o0 >= 64u ? ~0ull : (1ull << (n_entries - o0)) - 1ull; // bits at or beyond n_entries: ignored
        uint64_t bits = in_range;
        if (!ALL) {
            bits &= bitmap[tile]; // (the same 8 bytes in every lane; the bitmap is padded to whole 16-byte groups)
            if (bits == 0) continue;
        }
        const uint64_t o = o0 + lane;
        uint64_t key = ~0ull; // the global bin; all ones for a lane without an entry
        if (o < n_entries) {
            const uint32_t g = org[o];
            if (g < n_orgs) key = bin_base[g] + pos[o] / bin_width;
        }
        const uint32_t key_lo = (uint32_t)key, key_hi = (uint32_t)(key >> 32);
        const uint32_t prev_lo = (uint32_t)__shfl_up((int)key_lo, 1), prev_hi = (uint32_t)__shfl_up((int)key_hi, 1);
        const uint64_t heads = __ballot(lane == 0 || key_lo != prev_lo || key_hi != prev_hi);
        if ((heads >> lane) & 1ull) {
            const uint64_t behind = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
            const uint32_t end = behind ? (uint32_t)__builtin_ctzll(behind) : 64u;
            const uint32_t sum = (uint32_t)__popcll(bits & kid_cov_bits(lane, end));
            if (sum != 0 && key < n_bins) atomicAdd(&counts[key], sum);
        }
    }
}

// One wave per organism: its record from probes[] and seen[] of its bins.  For the longest run of occupied bins without
// a seen entry the chunks of 64 bins are folded left to right: `cur` is the run that reaches the end of the bins so far,
// a lane whose bin is seen and has another seen bin behind it in the chunk measures the run between the two.
__global__ __launch_bounds__(256) void kid_cov_reduce_kernel(const uint32_t *span, const unsigned long long *bin_base, const uint32_t *probes,
                                                             const uint32_t *seen, uint32_t n_orgs, KidCoverageRec *out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t g = wave0; g < n_orgs; g += n_waves) {
        const uint32_t nb = span[g];
        const uint64_t base = bin_base[g];
        uint32_t sum_p = 0, sum_s = 0, best_s = 0, best_b = 0, lane_gap = 0; // per lane
        uint32_t bins = 0, bins_seen = 0, cur = 0, gap = 0;                   // the same in every lane
        for (uint32_t c = 0; c < nb; c += 64u) {
            const uint32_t b = c + lane;
            uint32_t p = 0, s = 0;
            if (b < nb) { // (nb is at most the cap on all bins, 2^28: c + lane does not wrap)
                p = probes[base + b];
                s = seen[base + b];
            }
            sum_p += p;
            sum_s += s;
            if (s > best_s) { best_s = s; best_b = b; } // (b ascends in a lane: the lowest bin of a lane's maximum stays)
            const uint64_t occ = __ballot(p > 0), hit = __ballot(s > 0);
            bins += (uint32_t)__popcll(occ);
            bins_seen += (uint32_t)__popcll(hit);
            if (!hit) {
                cur += (uint32_t)__popcll(occ);
            } else {
                const uint32_t first = (uint32_t)__builtin_ctzll(hit), last = 63u - (uint32_t)__builtin_clzll(hit);
                cur += (uint32_t)__popcll(occ & kid_cov_bits(0, first));
                gap = cur > gap ? cur : gap;
                cur = (uint32_t)__popcll(occ & kid_cov_bits(last + 1u, 64u));
                if (s > 0 && lane != last) {
                    const uint64_t behind = hit & (~0ull << (lane + 1u)); // (lane < last <= 63)
                    const uint32_t run = (uint32_t)__popcll(occ & kid_cov_bits(lane + 1u, (uint32_t)__builtin_ctzll(behind)));
                    lane_gap = run > lane_gap ? run : lane_gap;
                }
            }
        }
        gap = cur > gap ? cur : gap;
        const uint32_t inner = kid_cov_wave_max(lane_gap);
        gap = inner > gap ? inner : gap;
        const uint32_t n_probes = kid_cov_wave_sum(sum_p), n_seen = kid_cov_wave_sum(sum_s);
        const uint32_t max_s = kid_cov_wave_max(best_s);
        // the lowest bin among the lanes that hold the maximum
        uint32_t cand = (best_s == max_s && max_s > 0) ? best_b : ~0u;
        for (int w = 32; w > 0; w >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)cand, w);
            cand = o < cand ? o : cand;
        }
        if (lane == 0) {
            KidCoverageRec r;
            r.n_probes = n_probes;
            r.n_seen = n_seen;
            r.span_bins = nb;
            r.bins = bins;
            r.bins_seen = bins_seen;
            r.max_gap = gap;
            r.max_bin_seen = max_s;
            r.max_bin = max_s > 0 ? cand : 0u;
            out[g] = r;
        }
    }
}
