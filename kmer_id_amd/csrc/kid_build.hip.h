// kid_build.hip.h -- device code of the probe-database builder (kmer_build_vf6).
//
// The table is 2^log2_cells uint32 cells, direct mapped by fmix64(canonical 30-mer) with no key stored:
// cell = target << 11 | count, 0 = empty, 1 = spoiled.  Three passes over ACGTN text (1 byte per base):
//   add     (phase 1)  every canonical 30-mer of an ingroup genome: a CAS loop that merges the genome's target into
//                      the cell (LCA) and bumps the count; it leaves without writing once the cell's target is <= 1
//   remove  (phase 2)  every 30-mer of an outgroup: a plain store of 1 over a live cell
//   claim   (phase 3)  three launches per batch: first occurrence of every live cell (atomicMin of the position into a
//                      batch-local side hash), the winners' filter (minct, entropy, "bad"), then every touched cell = 1
// A thread takes KID_BUILD_SEG consecutive k-mer end positions of a chunk and rolls the 29 bases in front of the first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kid_common.h"

#define KID_BUILD_K 30
#define KID_BUILD_SEG 16
#define KID_BUILD_BLOCK 256
#define KID_BUILD_REPSHIFT 11
#define KID_BUILD_MAXCOUNT 2047u

struct KidBuildCand {  // = kid_build_cand of include/kmer_id_amd.h
    uint64_t key;
    int64_t gpos;
    int32_t target;
    uint16_t count;
    uint8_t strand_r;
    uint8_t flags;
};

// Rolls the k-mers ending at [e0, e1) of text[0, n) (e1 <= n) and calls f(end, keyF, keyR) for every one of 30 ACGT bases.
template <class F>
__device__ __forceinline__ void kid_build_roll(const uint8_t *__restrict__ text, uint64_t e0, uint64_t e1, F &&f)
{
    const uint64_t mask = (1ull << (2 * KID_BUILD_K)) - 1;
    uint64_t kf = 0, kr = 0;
    int cpos = 0;
    for (uint64_t p = e0 >= KID_BUILD_K - 1 ? e0 - (KID_BUILD_K - 1) : 0; p < e1; ++p) {
        const uint8_t c = text[p];
        const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
        if (v > 3) {
            cpos = 0;
            kf = kr = 0;
            continue;
        }
        kf = ((kf << 2) & mask) | v;
        kr = (kr >> 2) | ((uint64_t)(3 - v) << (2 * (KID_BUILD_K - 1)));
        if (cpos < KID_BUILD_K) ++cpos;
        if (cpos == KID_BUILD_K && p >= e0) f(p, kf, kr);
    }
}

// Tree1::ca of the reference: the first node on y's path to the root that is 1 or on x's path (x's path: the nodes > 1
// met from x on).  parent[] entries are in [0, ntar); the walks are bounded so that a cyclic parent[] cannot hang.
__device__ __forceinline__ uint32_t kid_build_ca(const int32_t *__restrict__ parent, int32_t ntar, uint32_t x, uint32_t y)
{
    int32_t z = (int32_t)y;
    for (int32_t g = 0; g <= ntar; ++g) {
        if (z == 1) return 1;
        int32_t w = (int32_t)x;
        for (int32_t h = 0; w > 1 && h <= ntar; ++h) {
            if (w == z) return (uint32_t)z;
            w = parent[w];
        }
        z = parent[z];
    }
    return 1;
}

__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_add_kernel(uint32_t *table, uint64_t cell_mask, const uint8_t *__restrict__ text,
                                                                         uint64_t first, uint64_t n, uint32_t target,
                                                                         const int32_t *__restrict__ parent, int32_t ntar,
                                                                         unsigned long long *n_filled)
{
    const uint64_t e0 = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * KID_BUILD_SEG;
    if (e0 >= n) return;
    const uint64_t e1 = e0 + KID_BUILD_SEG < n ? e0 + KID_BUILD_SEG : n;
    uint32_t filled = 0;
    kid_build_roll(text, e0, e1, [&](uint64_t, uint64_t kf, uint64_t kr) {
        const uint64_t idx = kid_fmix64(kf < kr ? kf : kr) & cell_mask;
        uint32_t old = __hip_atomic_load(table + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
            uint32_t nv;
            if (old == 0) {
                nv = (target << KID_BUILD_REPSHIFT) | 1u;
            } else {
                const uint32_t t = old >> KID_BUILD_REPSHIFT, c = old & KID_BUILD_MAXCOUNT;
                if (t <= 1) break; // spoiled or at the root: the reference leaves it as it is
                nv = c == KID_BUILD_MAXCOUNT ? 1u : (kid_build_ca(parent, ntar, t, target) << KID_BUILD_REPSHIFT) | (c + 1);
            }
            const uint32_t prev = atomicCAS(table + idx, old, nv);
            if (prev == old) {
                filled += old == 0;
                break;
            }
            old = prev;
        }
    });
    if (filled) atomicAdd(n_filled, (unsigned long long)filled);
}

__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_remove_kernel(uint32_t *table, uint64_t cell_mask, const uint8_t *__restrict__ text,
                                                                            uint64_t first, uint64_t n)
{
    const uint64_t e0 = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * KID_BUILD_SEG;
    if (e0 >= n) return;
    const uint64_t e1 = e0 + KID_BUILD_SEG < n ? e0 + KID_BUILD_SEG : n;
    kid_build_roll(text, e0, e1, [&](uint64_t, uint64_t kf, uint64_t kr) {
        const uint64_t idx = kid_fmix64(kf < kr ? kf : kr) & cell_mask;
        if (table[idx] > 1) table[idx] = 1;
    });
}

// side hash of a claim batch: key = cell index + 1 (0 = free), value = smallest end position that met the cell
__device__ __forceinline__ uint64_t kid_build_side_slot(uint64_t idx, uint64_t side_mask) { return kid_fmix64(idx + 1) & side_mask; }

__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_claim_kernel(const uint32_t *__restrict__ table, uint64_t cell_mask,
                                                                           const uint8_t *__restrict__ text, uint64_t first, uint64_t n,
                                                                           unsigned long long *side_key, uint32_t *side_pos, uint64_t side_mask)
{
    const uint64_t e0 = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * KID_BUILD_SEG;
    if (e0 >= n) return;
    const uint64_t e1 = e0 + KID_BUILD_SEG < n ? e0 + KID_BUILD_SEG : n;
    kid_build_roll(text, e0, e1, [&](uint64_t e, uint64_t kf, uint64_t kr) {
        const uint64_t idx = kid_fmix64(kf < kr ? kf : kr) & cell_mask;
        if (table[idx] <= 1) return;
        // at most one live k-mer per end position and the side hash has >= 2 slots per position: a free slot exists
        for (uint64_t h = kid_build_side_slot(idx, side_mask);; h = (h + 1) & side_mask) {
            const unsigned long long k = atomicCAS(side_key + h, 0ull, (unsigned long long)(idx + 1));
            if (k == 0 || k == idx + 1) {
                atomicMin(side_pos + h, (uint32_t)e);
                break;
            }
        }
    });
}

// check_entropy of the reference for the 30-mer `key`.  The frame totals are fixed (19, 14 and 10 with the pseudo-counts),
// so every p*log10(p) comes from a host table (term[20*f + n], f = 0,1,2 for mod 2,3,5, n = count + 1): the device only
// subtracts, adds and divides, in the reference's order.  Returns bit 0 = passes, bit 1 = "bad" (printed by the host).
__device__ __forceinline__ uint32_t kid_build_entropy(uint64_t key, const double *__restrict__ term, double log10_4)
{
    uint32_t fr[10]; // 4 counts of 8 bits per frame; every index below is a constant once the loop is unrolled
#pragma unroll
    for (int j = 0; j < 10; ++j) fr[j] = 0x01010101u; // pseudo-counts
    int row = 0, maxrow = 0;
    uint32_t prev = 4;
#pragma unroll
    for (int i = 0; i < KID_BUILD_K; ++i) {
        const uint32_t b = (uint32_t)(key >> (2 * (KID_BUILD_K - 1 - i))) & 3u;
        if (b == prev) {
            ++row;
            maxrow = row > maxrow ? row : maxrow;
        } else {
            row = 1;
            prev = b;
        }
        const uint32_t one = 1u << (8 * b);
        fr[i % 2] += one;
        fr[i % 3 + 2] += one;
        fr[i % 5 + 5] += one;
    }
    if (maxrow > 11) return 0;
    double ent[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const double *t = term + 20 * (j < 2 ? 0 : j < 5 ? 1 : 2);
        double e = -t[fr[j] & 255u];
        e = e - t[(fr[j] >> 8) & 255u];
        e = e - t[(fr[j] >> 16) & 255u];
        e = e - t[fr[j] >> 24];
        ent[j] = e;
    }
    const double e2 = (ent[0] + ent[1]) / 2.0 / log10_4;
    const double e3 = (ent[2] + ent[3] + ent[4]) / 3.0 / log10_4;
    const double e5 = (ent[5] + ent[6] + ent[7] + ent[8] + ent[9]) / 5.0 / log10_4;
    if (e2 < 0.80 || e3 < 0.80 || e5 < 0.80) return 0;
    const bool bad = (key & 0x3333333333333333ull) == 0 || (key & 0xCCCCCCCCCCCCCCCCull) == 0;
    return 1u | (bad ? 2u : 0u);
}

__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_filter_kernel(const uint32_t *__restrict__ table, uint64_t cell_mask,
                                                                            const uint8_t *__restrict__ text, uint64_t first, uint64_t n,
                                                                            int64_t gpos_base, const unsigned long long *__restrict__ side_key,
                                                                            const uint32_t *__restrict__ side_pos, uint64_t side_mask,
                                                                            const int32_t *__restrict__ minct, const double *__restrict__ term,
                                                                            double log10_4, KidBuildCand *cand, unsigned long long *n_cand,
                                                                            uint64_t cap)
{
    const uint64_t e0 = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * KID_BUILD_SEG;
    if (e0 >= n) return;
    const uint64_t e1 = e0 + KID_BUILD_SEG < n ? e0 + KID_BUILD_SEG : n;
    kid_build_roll(text, e0, e1, [&](uint64_t e, uint64_t kf, uint64_t kr) {
        const uint64_t key = kf < kr ? kf : kr;
        const uint64_t idx = kid_fmix64(key) & cell_mask;
        const uint32_t v = table[idx];
        if (v <= 1) return;
        uint64_t h = kid_build_side_slot(idx, side_mask);
        while (side_key[h] != idx + 1) h = (h + 1) & side_mask; // the claim pass put it there
        if (side_pos[h] != (uint32_t)e) return;                  // not the first occurrence in this batch
        const uint32_t t = v >> KID_BUILD_REPSHIFT, c = v & KID_BUILD_MAXCOUNT;
        if (t <= 1 || (int32_t)c < minct[t]) return;
        const unsigned long long slot = atomicAdd(n_cand, 1ull);
        if (slot >= cap) return;
        KidBuildCand o;
        o.key = key;
        o.gpos = gpos_base + (int64_t)e;
        o.target = (int32_t)t;
        o.count = (uint16_t)c;
        o.strand_r = kf < kr ? 0 : 1;
        o.flags = (uint8_t)kid_build_entropy(key, term, log10_4);
        cand[slot] = o;
    });
}

__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_mark_kernel(uint32_t *table, uint64_t cell_mask, const uint8_t *__restrict__ text,
                                                                          uint64_t first, uint64_t n)
{
    const uint64_t e0 = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * KID_BUILD_SEG;
    if (e0 >= n) return;
    const uint64_t e1 = e0 + KID_BUILD_SEG < n ? e0 + KID_BUILD_SEG : n;
    kid_build_roll(text, e0, e1, [&](uint64_t, uint64_t kf, uint64_t kr) { table[kid_fmix64(kf < kr ? kf : kr) & cell_mask] = 1; });
}

// The digest plane of a finished minimizer-localised table (kid_common.h): one thread per line, headers only -- 16 of
// every 128 bytes asked for, but whole lines fetched: a pass over the table, ~3.4 ms for 16 GiB.  Runs behind
// kid_build_firstwins_kernel, which leaves the headers as kid_build_insert_kernel wrote them.
__global__ __launch_bounds__(KID_BUILD_BLOCK) void kid_build_digest_kernel(const uint4 *__restrict__ table, uint64_t n_lines, uint2 *__restrict__ digest)
{
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n_lines; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 h = table[l * KID_LINE_CELLS];
        uint2 d;
        kid_digest_of_header(h.x, h.y, h.z, h.w, d.x, d.y);
        digest[l] = d;
    }
}

__global__ void kid_build_entropy_kernel(const uint64_t *__restrict__ keys, uint64_t n, const double *__restrict__ term, double log10_4,
                                         uint8_t *flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        flags[i] = (uint8_t)kid_build_entropy(keys[i], term, log10_4);
}
