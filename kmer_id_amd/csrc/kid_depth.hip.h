// kid_depth.hip.h -- k-mer depth per database entry (KID_OPT_ENTRY_DEPTH): the counter the tally variant of
// kid_support_kernel adds to, and the kernels that reduce a counter array to a per-target depth spectrum.
//   depth[o]          how often entry o was hit by the reads a tally counted with confident > 0 (uint32, saturating);
//                     the numbering of the seen-bitmap and of kid_hit.entry, padded with zeros like ord_target
//   spectrum[t][b]    entries of target t with depth b (b < bins - 1), or depth >= bins - 1 (the last column)
//   ksum[t], dmax[t]  sum and maximum of depth over the entries of target t
// The counters are almost all zero in a metagenomic sample: the spectrum kernel streams them 16 bytes per lane (as
// kid_ucount_kernel streams the bitmap) and looks up ord_target only for the non-zero ones; column 0 is what is left of
// the target's entries (kid_depth_entries_kernel, once per database).  Equal targets and equal (target, bin) pairs are
// merged inside the wave before the global atomics.  Integer sums: the output does not depend on the order of the adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KID_DEPTH_MAX 0xFFFFFFFFu
#define KID_DEPTH_MAX_BINS 4096u

// depth[entry]++, saturating: the add that wrapped the counter (it read the maximum) puts the maximum back.  Adds that
// land between the two read small values and are lost, as they should be; an add behind the atomicMax reads the maximum
// and repairs its own wrap -- so the last operation on a saturated counter always leaves the maximum.
__device__ __forceinline__ void kid_depth_count(uint32_t *depth, uint32_t entry)
{
    if (atomicAdd(&depth[entry], 1u) == KID_DEPTH_MAX) atomicMax(&depth[entry], KID_DEPTH_MAX);
}

// dst[i] = min(dst[i] + src[i], 2^32 - 1): the merge of two samples' counters (nothing else writes dst meanwhile)
__global__ void kid_depth_add_kernel(uint32_t *dst, const uint32_t *src, uint64_t n)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = dst[i], s = a + src[i];
        dst[i] = s < a ? KID_DEPTH_MAX : s;
    }
}

// per_target[t] = entries o < n_entries with ord_target[o] == t.  Entries of one target mostly lie in runs: a wave adds
// one number per run of its 64 entries (any order of targets is counted right: a run may be one entry long).
__global__ __launch_bounds__(256) void kid_depth_entries_kernel(const uint32_t *ord_target, uint64_t n_entries, uint32_t ntar,
                                                                 unsigned long long *per_target)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t o0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; o0 < n_entries; o0 += n_waves * 64u) {
        const uint64_t o = o0 + lane;
        const bool have = o < n_entries;
        const uint32_t t = have ? ord_target[o] : 0u;
        const uint32_t prev = (uint32_t)__shfl_up((int)t, 1);
        const uint64_t valid = __ballot(have); // the lanes 0 .. n - 1
        const uint64_t heads = __ballot(have && (lane == 0 || prev != t));
        if (have && ((heads >> lane) & 1ull) && t < ntar) {
            const uint64_t above = (heads >> lane) >> 1; // the run ends in front of the next head, or with the last entry
            const uint32_t end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : (uint32_t)__popcll(valid);
            atomicAdd(&per_target[t], (unsigned long long)(end - lane));
        }
    }
}

// the columns 1 .. bins - 1 of the spectrum, ksum and dmax from the non-zero counters of depth[0 .. 4 * n_quads)
__global__ __launch_bounds__(256) void kid_depth_spectrum_kernel(const uint32_t *depth, uint64_t n_quads, const uint32_t *ord_target,
                                                                  uint32_t ntar, uint32_t bins, unsigned long long *spectrum,
                                                                  unsigned long long *ksum, uint32_t *dmax)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    const uint4 *depth4 = reinterpret_cast<const uint4 *>(depth);
    for (uint64_t q0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; q0 < n_quads; q0 += n_waves * 64u) {
        const uint64_t q = q0 + lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < n_quads) v = depth4[q];
        if (__ballot((v.x | v.y | v.z | v.w) != 0) == 0) continue;
        const uint32_t d4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t d = d4[i];
            uint32_t t = 0;
            if (d != 0) t = ord_target[q * 4ull + (uint64_t)i];
            const bool act = d != 0 && t < ntar;
            const uint32_t b = d < bins - 1u ? d : bins - 1u;
            uint64_t todo = __ballot(act);
            while (todo) { // one round per target among the wave's non-zero counters: mostly one
                const int j = __builtin_ctzll(todo);
                const uint32_t tj = (uint32_t)__builtin_amdgcn_readlane((int)t, j);
                const uint64_t peers = __ballot(act && t == tj);
                todo &= ~peers;
                const bool mine = (peers >> lane) & 1ull;
                unsigned long long s = mine ? (unsigned long long)d : 0ull;
                uint32_t mx = mine ? d : 0u;
#pragma unroll
                for (int w = 32; w >= 1; w >>= 1) {
                    s += __shfl_xor(s, w);
                    const uint32_t o = (uint32_t)__shfl_xor((int)mx, w);
                    mx = mx > o ? mx : o;
                }
                if (lane == (uint32_t)j) {
                    atomicAdd(&ksum[tj], s);
                    atomicMax(&dmax[tj], mx);
                }
                uint64_t left = peers; // ... and one add per bin among them
                while (left) {
                    const int l = __builtin_ctzll(left);
                    const uint32_t bl = (uint32_t)__builtin_amdgcn_readlane((int)b, l);
                    const uint64_t same = __ballot(mine && b == bl);
                    left &= ~same;
                    if (lane == (uint32_t)l) atomicAdd(&spectrum[(uint64_t)tj * bins + bl], (unsigned long long)__popcll(same));
                }
            }
        }
    }
}

// column 0: the target's entries that are in no other column.  One wave per target.
__global__ __launch_bounds__(256) void kid_depth_column0_kernel(unsigned long long *spectrum, const unsigned long long *per_target,
                                                                 uint32_t ntar, uint32_t bins)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6); t < ntar; t += gridDim.x * 4u) {
        unsigned long long s = 0;
        for (uint32_t b = 1u + lane; b < bins; b += 64u) s += spectrum[(uint64_t)t * bins + b];
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w);
        if (lane == 0) spectrum[(uint64_t)t * bins] = per_target[t] - s;
    }
}
