// kid_pileup.hip.h -- placed reads piled up per genome bin: two uint32 counters per bin, `starts` and `depth`, from the
// kid_locus records of kid_loci.hip.h (include/kmer_id_amd.h has the rule).  The geometry is that of kid_coverage.hip.h for
// the same bin width W (kid_cov_span_kernel and kid_cov_scan_kernel make it): span_bins[g], bin_base, B bins.
// depth is kept as a STEP array: organism g owns the span_bins[g] + 1 slots from bin_base[g] + g on, the last of them a
// sentinel; a record over the bins b_lo..b_hi adds +1 to slot b_lo and -1 (uint32 wrap-around) to slot b_hi + 1, which is
// the sentinel when b_hi is the organism's last bin and never a slot of the next organism.  The steps of an organism sum
// to zero, so ONE unsegmented inclusive scan over all B + n_orgs slots is every organism's depth, and a record costs
// three atomics whatever its chain spans.
//   add     kid_pileup_add_kernel, once per record type (kid_locus, or the kid_fragment_locus of kid_fragment_loci.hip.h,
//           which carries its interval: kid_pileup_interval): one lane per record; the lanes of a wave whose slot is that of the lane before them
//           form a run, and the head of a run issues one atomicAdd of the run's length (every read on one locus, or a
//           sorted input: one atomic per wave and array instead of 64 on one address).  Runs are an optimisation only.
//   scan    kid_pileup_tile_sum_kernel, kid_pileup_tile_scan_kernel (one workgroup), kid_pileup_apply_kernel: ordered by
//           kernel boundaries.  No look-back, no flag another workgroup spins on, no fence.  The steps are only read.
//   reduce  kid_pileup_reduce_kernel: one wave per organism walks its bins 64 at a time, folds max_gap left to right and
//           writes the organism's record; it also leaves depth in the layout of `starts` when asked to.
// All arithmetic on counters is uint32 and commutative: the result does not depend on any order of work.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kid_coverage.hip.h"
#include "kid_fragment_loci.hip.h"
#include "kid_loci.hip.h"

#define KID_PILEUP_SCAN_TILE 2048u // slots per tile of the scan: 256 threads, 8 slots each
#define KID_PILEUP_REC_WORDS 12u   // kid_pileup_rec: nine uint32, a word of padding, the two halves of depth_sum: 48 bytes

// the sites and the geometry a pileup was made for
struct KidPileupGeo {
    const uint32_t *org, *pos; // per entry
    uint64_t n_entries;
    const uint32_t *span;               // [n_orgs]
    const unsigned long long *bin_base; // [n_orgs + 1]
    uint32_t n_orgs, bin_width, k;
};

// One atomicAdd per run of equal keys in a wave: key ~0 is "nothing to add".  what: the value one lane adds.
__device__ __forceinline__ void kid_pileup_add_runs(uint32_t *a, uint64_t key, uint64_t shift, uint32_t what, uint32_t lane)
{
    const uint32_t key_lo = (uint32_t)key, key_hi = (uint32_t)(key >> 32);
    const uint32_t prev_lo = (uint32_t)__shfl_up((int)key_lo, 1), prev_hi = (uint32_t)__shfl_up((int)key_hi, 1);
    const uint64_t heads = __ballot(lane == 0 || key_lo != prev_lo || key_hi != prev_hi);
    if (((heads >> lane) & 1ull) && key != ~0ull) {
        const uint64_t behind = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
        const uint32_t end = behind ? (uint32_t)__builtin_ctzll(behind) : 64u;
        atomicAdd(&a[key - shift], what * (end - lane));
    }
}

struct KidPileupRule {
    uint32_t min_chain, min_margin;
    uint32_t paired_only; // fragment records alone: 1 places none but those with both mates
};

// Is the record placed, and where: its organism and the two ends of its genome interval.  One overload per record type.
__device__ __forceinline__ bool kid_pileup_interval(const KidLocus &L, const KidPileupGeo &geo, const KidPileupRule &rule, uint32_t &org, int64_t &lo,
                                                    int64_t &hi)
{
    const uint32_t margin = L.n_chain >= L.n_other ? L.n_chain - L.n_other : 0u;
    if (!(L.n_chain >= rule.min_chain && margin >= rule.min_margin && L.strand <= 1u && L.entry_first < geo.n_entries &&
          L.org == geo.org[L.entry_first] && L.org < geo.n_orgs))
        return false;
    const int64_t a = (int64_t)geo.pos[L.entry_first];
    const int64_t d = L.pos_last >= L.pos_first ? (int64_t)(L.pos_last - L.pos_first) : 0;
    if (L.strand == 0u) {
        lo = a;
        hi = a + d + (int64_t)geo.k - 1;
    } else {
        lo = a - d > 0 ? a - d : 0;
        hi = a + (int64_t)geo.k - 1;
    }
    org = L.org;
    return true;
}

// (a fragment record carries its interval: the sites are not looked at)
__device__ __forceinline__ bool kid_pileup_interval(const KidFragmentLocus &L, const KidPileupGeo &geo, const KidPileupRule &rule, uint32_t &org,
                                                    int64_t &lo, int64_t &hi)
{
    const uint32_t margin = L.n_chain >= L.n_other ? L.n_chain - L.n_other : 0u;
    if (!(L.mates >= 1u && L.mates <= 3u && (!rule.paired_only || L.mates == 3u) && L.n_chain >= rule.min_chain && margin >= rule.min_margin &&
          L.org < geo.n_orgs && L.lo <= L.hi))
        return false;
    lo = (int64_t)L.lo;
    hi = (int64_t)L.hi;
    org = L.org;
    return true;
}

// counts: [0] records handed in, [1] records placed (one atomic per wave and counter)
template <class Rec>
__global__ __launch_bounds__(256) void kid_pileup_add_kernel(const Rec *loci, uint64_t n, KidPileupGeo geo, KidPileupRule rule, uint32_t *starts,
                                                             uint32_t *steps, unsigned long long *counts)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride; // (the same in every lane: no lane leaves before a shuffle)
    uint32_t seen = 0, placed = 0;                     // of this wave (the same in every lane)
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t slot_lo = ~0ull, slot_hi1 = ~0ull, g = 0;
        if (i < n) {
            const Rec L = loci[i];
            uint32_t org;
            int64_t lo, hi;
            if (kid_pileup_interval(L, geo, rule, org, lo, hi)) {
                const uint32_t nb = geo.span[org];
                if (nb >= 1u) { // (an organism with an entry has a bin)
                    uint64_t b_lo = (uint64_t)lo / geo.bin_width, b_hi = (uint64_t)hi / geo.bin_width;
                    b_lo = b_lo < nb - 1u ? b_lo : nb - 1u;
                    b_hi = b_hi < nb - 1u ? b_hi : nb - 1u;
                    g = org;
                    const uint64_t base = geo.bin_base[g] + g; // the organism's first slot
                    slot_lo = base + b_lo;
                    slot_hi1 = base + b_hi + 1u; // at most the sentinel, base + nb
                }
            }
        }
        seen += (uint32_t)__popcll(__ballot(i < n));
        placed += (uint32_t)__popcll(__ballot(slot_lo != ~0ull));
        // (a slot belongs to one organism: the lanes of a run share g, and slot - g is the bin's place in `starts`)
        kid_pileup_add_runs(starts, slot_lo, g, 1u, lane);
        kid_pileup_add_runs(steps, slot_lo, 0, 1u, lane);
        kid_pileup_add_runs(steps, slot_hi1, 0, ~0u, lane);
    }
    if (lane == 0) {
        if (seen) atomicAdd(&counts[0], (unsigned long long)seen);
        if (placed) atomicAdd(&counts[1], (unsigned long long)placed);
    }
}

// dst[i] += src[i] with wrap-around: starts and steps are linear, so the pileup of a union is the sum of the parts'
__global__ __launch_bounds__(256) void kid_pileup_merge_kernel(const uint32_t *src, uint64_t n, uint32_t *dst)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] += src[i];
}

// ---------------------------------------------------------------- the scan of the steps
// inclusive scan of one value per thread over the 256 threads of a workgroup; *total: the sum of all (part: 4 words of LDS)
__device__ __forceinline__ uint32_t kid_pileup_wg_scan(uint32_t v, uint32_t *part, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int w = 1; w < 64; w <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, w);
        if (lane >= (uint32_t)w) v += o;
    }
    __syncthreads(); // (part may still be read from the call before)
    if (lane == 63u) part[wave] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 4u; w++) {
        const uint32_t p = part[w];
        before += w < wave ? p : 0u;
        all += p;
    }
    *total = all;
    return v + before;
}

// tile_sums[t] = the sum of the slots of tile t
__global__ __launch_bounds__(256) void kid_pileup_tile_sum_kernel(const uint32_t *steps, uint64_t n_slots, uint64_t n_tiles, uint32_t *tile_sums)
{
    __shared__ uint32_t part[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t s0 = t * KID_PILEUP_SCAN_TILE + (uint64_t)threadIdx.x * 8u;
        uint32_t sum = 0;
        for (uint32_t j = 0; j < 8u; j++)
            if (s0 + j < n_slots) sum += steps[s0 + j];
        uint32_t total;
        (void)kid_pileup_wg_scan(sum, part, &total);
        if (threadIdx.x == 0) tile_sums[t] = total;
    }
}

// tile_sums[t] <- tile_sums[0] + ... + tile_sums[t - 1], by one workgroup, KID_PILEUP_SCAN_TILE sums at a time
__global__ __launch_bounds__(256) void kid_pileup_tile_scan_kernel(uint32_t *tile_sums, uint64_t n_tiles)
{
    __shared__ uint32_t part[4];
    uint32_t carry = 0;
    for (uint64_t c = 0; c < n_tiles; c += KID_PILEUP_SCAN_TILE) {
        const uint64_t t0 = c + (uint64_t)threadIdx.x * 8u;
        uint32_t v[8], sum = 0;
        for (uint32_t j = 0; j < 8u; j++) {
            v[j] = t0 + j < n_tiles ? tile_sums[t0 + j] : 0u;
            sum += v[j];
        }
        uint32_t total;
        uint32_t run = carry + kid_pileup_wg_scan(sum, part, &total) - sum;
        for (uint32_t j = 0; j < 8u; j++) {
            if (t0 + j < n_tiles) tile_sums[t0 + j] = run;
            run += v[j];
        }
        carry += total;
    }
}

// depth[s] = steps[0] + ... + steps[s]; tile_offsets: what the kernel above left
__global__ __launch_bounds__(256) void kid_pileup_apply_kernel(const uint32_t *steps, uint64_t n_slots, uint64_t n_tiles,
                                                               const uint32_t *tile_offsets, uint32_t *depth)
{
    __shared__ uint32_t part[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t s0 = t * KID_PILEUP_SCAN_TILE + (uint64_t)threadIdx.x * 8u;
        uint32_t v[8], sum = 0;
        for (uint32_t j = 0; j < 8u; j++) {
            v[j] = s0 + j < n_slots ? steps[s0 + j] : 0u;
            sum += v[j];
        }
        uint32_t total;
        uint32_t run = tile_offsets[t] + kid_pileup_wg_scan(sum, part, &total) - sum;
        for (uint32_t j = 0; j < 8u; j++) {
            run += v[j];
            if (s0 + j < n_slots) depth[s0 + j] = run;
        }
    }
}

// ---------------------------------------------------------------- one record per organism
// the longest run of set bits of m
__device__ __forceinline__ uint32_t kid_pileup_longest_run(uint64_t m)
{
    uint32_t n = 0;
    while (m) {
        m &= m << 1;
        n++;
    }
    return n;
}

// the largest value over the wave and the lowest `at` among the lanes that hold it (0, 0 when the largest is 0)
__device__ __forceinline__ void kid_pileup_wave_argmax(uint32_t best, uint32_t at, uint32_t *max_out, uint32_t *at_out)
{
    const uint32_t m = kid_cov_wave_max(best);
    uint32_t cand = (best == m && m > 0) ? at : ~0u;
    for (int w = 32; w > 0; w >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)cand, w);
        cand = o < cand ? o : cand;
    }
    *max_out = m;
    *at_out = m > 0 ? cand : 0u;
}

// starts: [B] at bin_base[g]; depth: the scanned slots, organism g's at bin_base[g] + g.  out: KID_PILEUP_REC_WORDS words
// per organism, or null; depth_bins: depth in the layout of `starts`, or null.
__global__ __launch_bounds__(256) void kid_pileup_reduce_kernel(const uint32_t *span, const unsigned long long *bin_base, const uint32_t *starts,
                                                                const uint32_t *depth, uint32_t n_orgs, uint32_t *out, uint32_t *depth_bins)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t g = wave0; g < n_orgs; g += n_waves) {
        const uint32_t nb = span[g];
        const uint64_t base = bin_base[g];
        uint32_t sum_s = 0, best_s = 0, best_s_at = 0, best_d = 0, best_d_at = 0; // per lane
        uint64_t sum_d = 0;                                                         // per lane
        uint32_t covered = 0, cur = 0, gap = 0;                                     // the same in every lane
        for (uint32_t c = 0; c < nb; c += 64u) {
            const uint32_t b = c + lane; // (nb is at most the cap on all bins, 2^28: c + lane does not wrap)
            uint32_t s = 0, d = 0;
            if (b < nb) {
                s = starts[base + b];
                d = depth[base + g + b];
                if (depth_bins) depth_bins[base + b] = d;
            }
            sum_s += s;
            sum_d += d;
            if (s > best_s) { best_s = s; best_s_at = b; } // (b ascends in a lane: the lowest bin of a lane's maximum stays)
            if (d > best_d) { best_d = d; best_d_at = b; }
            const uint64_t valid = kid_cov_bits(0, nb - c < 64u ? nb - c : 64u);
            const uint64_t full = __ballot(d > 0), empty = valid & ~full;
            covered += (uint32_t)__popcll(full);
            if (!full) {
                cur += (uint32_t)__popcll(valid);
            } else {
                const uint32_t first = (uint32_t)__builtin_ctzll(full), last = 63u - (uint32_t)__builtin_clzll(full);
                cur += first;
                gap = cur > gap ? cur : gap;
                cur = (uint32_t)__popcll(valid) - 1u - last;
                const uint32_t inner = kid_pileup_longest_run(empty & kid_cov_bits(first, last));
                gap = inner > gap ? inner : gap;
            }
        }
        gap = cur > gap ? cur : gap;
        const uint32_t n_placed = kid_cov_wave_sum(sum_s);
        const uint32_t sum_lo = kid_cov_wave_sum((uint32_t)sum_d & 0xFFFFu), sum_mid = kid_cov_wave_sum((uint32_t)(sum_d >> 16) & 0xFFFFu);
        const uint32_t sum_top = kid_cov_wave_sum((uint32_t)(sum_d >> 32)); // (three parts that cannot overflow 32 bits over 64 lanes)
        const uint64_t depth_sum = (uint64_t)sum_lo + ((uint64_t)sum_mid << 16) + ((uint64_t)sum_top << 32);
        uint32_t max_d, max_d_at, max_s, max_s_at;
        kid_pileup_wave_argmax(best_d, best_d_at, &max_d, &max_d_at);
        kid_pileup_wave_argmax(best_s, best_s_at, &max_s, &max_s_at);
        if (out) { // the record's twelve words by twelve lanes: nine uint32, a word of padding, depth_sum low half first
            uint32_t v = 0;
            v = lane == 0u ? n_placed : v;
            v = lane == 1u ? nb : v;
            v = lane == 2u ? covered : v;
            v = lane == 3u ? gap : v;
            v = lane == 4u ? max_d : v;
            v = lane == 5u ? max_d_at : v;
            v = lane == 6u ? max_s : v;
            v = lane == 7u ? max_s_at : v;
            v = lane == 10u ? (uint32_t)depth_sum : v;
            v = lane == 11u ? (uint32_t)(depth_sum >> 32) : v;
            if (lane < KID_PILEUP_REC_WORDS) out[g * KID_PILEUP_REC_WORDS + lane] = v;
        }
    }
}
