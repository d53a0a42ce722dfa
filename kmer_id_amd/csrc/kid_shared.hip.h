// kid_shared.hip.h -- k-mers shared between samples: for n seen-bitmaps (the layout of kid_sample_seen_export: bit o is
// bit o % 32 of 32-bit word o / 32) and the entry -> target map ord_target,
//   shared[i][j][t] = #{ o < n_entries : bit o of b_i and of b_j set, ord_target[o] == t }      (64-bit sums)
// for every pair in ONE pass over the entries: a workgroup takes a contiguous span of tiles of KID_SHARED_TILE entries;
// per tile it brings the n samples' 64 words into LDS, reads ord_target for the tile once (not at all for a tile in which
// no sample has a bit), marks where the target changes and, run by run, adds popcount(b_i & b_j & run mask) for the pairs
// i <= j dealt over its lanes.  The sums stay in registers while the target stays the same, across tiles too, and go to
// global memory with one atomicAdd per non-zero (pair, target) when it changes or the span ends.  Runs are an
// optimisation only: any order of targets is counted right (a run may be one entry long, which is slow).  Bits at or
// beyond n_entries are masked by index.  kid_shared_mirror_kernel copies the triangle i < j to j > i.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef KID_SHARED_MAX_SAMPLES
#define KID_SHARED_MAX_SAMPLES 64    // (include/kmer_id_amd.h has it for the callers)
#endif
#define KID_SHARED_TILE 2048u        // entries per tile: 64 words = 16 quads of 16 bytes per sample
#define KID_SHARED_MIN_SPAN 4u       // tiles a workgroup takes at least (a small database still carries sums across tiles)
#define KID_SHARED_ROW 68u           // words per sample in LDS: 64 + 4, so that lanes on consecutive samples read different banks
#define KID_SHARED_SLOTS 9           // pairs per lane: 64 * 65 / 2 = 2080 pairs over 256 lanes

// the first head at or behind `pos` in the tile's head bitmap (words: which of its words hold one), or the tile's size
__device__ __forceinline__ uint32_t kid_shared_next_head(const uint32_t *heads, uint64_t words, uint32_t pos)
{
    if (pos >= KID_SHARED_TILE) return KID_SHARED_TILE;
    const uint32_t w = pos >> 5;
    const uint32_t m = heads[w] & (~0u << (pos & 31u));
    if (m) return w * 32u + (uint32_t)__builtin_ctz(m);
    const uint64_t rest = w < 63u ? words & (~0ull << (w + 1u)) : 0ull;
    if (!rest) return KID_SHARED_TILE;
    const uint32_t w2 = (uint32_t)__builtin_ctzll(rest);
    return w2 * 32u + (uint32_t)__builtin_ctz(heads[w2]);
}

// the bits [s, e) of the tile that fall into the word starting at bit `lo` (s, e, lo the same in every lane)
__device__ __forceinline__ uint32_t kid_shared_word_mask(uint32_t s, uint32_t e, uint32_t lo)
{
    const uint32_t a = s > lo ? (s - lo < 32u ? s - lo : 32u) : 0u;
    const uint32_t b = e > lo ? (e - lo < 32u ? e - lo : 32u) : 0u;
    if (b <= a) return 0u;
    const uint32_t upto_b = b == 32u ? ~0u : (1u << b) - 1u;
    return upto_b & ~((1u << a) - 1u); // (a < 32 here)
}

// split: lanes that share a pair (a power of two up to 16; split * pairs <= 256 when split > 1): each takes every
// split-th quad of the tile, and they add their sums up before the atomicAdd
__global__ __launch_bounds__(256) void kid_shared_kernel(const uint32_t *const *bitmaps, uint32_t n, uint64_t n_words,
                                                         const uint32_t *ord_target, uint64_t n_entries, uint32_t ntar,
                                                         uint64_t n_tiles, uint64_t span, uint32_t split,
                                                         unsigned long long *shared)
{
    __shared__ __attribute__((aligned(16))) uint32_t bits[KID_SHARED_MAX_SAMPLES * KID_SHARED_ROW];
    __shared__ __attribute__((aligned(16))) uint32_t targ[KID_SHARED_TILE];
    __shared__ uint32_t heads[KID_SHARED_TILE / 32u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t npairs = n * (n + 1u) / 2u;
    const uint32_t sub = tid & (split - 1u), pair0 = tid / split, pair_step = 256u / split;
    // this lane's pairs (i <= j, row by row): i | j << 8, or all ones for a slot without a pair
    uint32_t pij[KID_SHARED_SLOTS], acc[KID_SHARED_SLOTS];
#pragma unroll
    for (int k = 0; k < KID_SHARED_SLOTS; k++) {
        uint32_t p = pair0 + (uint32_t)k * pair_step, i = 0;
        pij[k] = ~0u;
        acc[k] = 0;
        if (p < npairs) {
            while (p >= n - i) { p -= n - i; i++; }
            pij[k] = i | (i + p) << 8;
        }
    }
    uint32_t cur_t = ~0u; // the target the sums belong to
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < KID_SHARED_SLOTS; k++) {
            uint32_t a = acc[k];
            for (uint32_t w = 1; w < split; w <<= 1) a += (uint32_t)__shfl_xor((int)a, (int)w);
            if (a != 0 && sub == 0 && pij[k] != ~0u && cur_t < ntar)
                atomicAdd(&shared[((uint64_t)(pij[k] & 255u) * n + (pij[k] >> 8)) * ntar + cur_t], (unsigned long long)a);
            acc[k] = 0;
        }
    };
    const uint64_t tile_begin = (uint64_t)blockIdx.x * span;
    const uint64_t tile_end = tile_begin + span < n_tiles ? tile_begin + span : n_tiles;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t o0 = tile * KID_SHARED_TILE, w0 = tile * (KID_SHARED_TILE / 32u);
        // ---- the samples' words of the tile -> LDS, 16 bytes per lane (words behind the bitmap's end: zero)
        uint32_t any = 0;
        for (uint32_t x = tid; x < n * 16u; x += 256u) {
            const uint32_t smp = x >> 4, quad = x & 15u;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w0 + quad * 4u < n_words) v = *reinterpret_cast<const uint4 *>(bitmaps[smp] + w0 + quad * 4u);
            *reinterpret_cast<uint4 *>(&bits[smp * KID_SHARED_ROW + quad * 4u]) = v;
            any |= v.x | v.y | v.z | v.w;
        }
        // (nothing reads `bits` in a tile that is skipped, and a tile that is not ends with a barrier: the next tile's
        // words never overwrite words a lane still counts)
        if (!__syncthreads_or((int)(any != 0))) continue;
        // ---- the tile's targets -> LDS, and where they change
        const uint32_t vend = n_entries - o0 < KID_SHARED_TILE ? (uint32_t)(n_entries - o0) : KID_SHARED_TILE; // entries of the tile
        for (uint32_t x = tid; x < KID_SHARED_TILE / 4u; x += 256u) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (o0 + x * 4u < n_words * 32u) v = *reinterpret_cast<const uint4 *>(ord_target + o0 + x * 4u);
            *reinterpret_cast<uint4 *>(&targ[x * 4u]) = v;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t c = 0; c < KID_SHARED_TILE / 256u; c++) {
            const uint32_t e = c * 256u + tid;
            const bool head = e < vend && (e == 0 || targ[e] != targ[e - 1u]);
            const uint64_t m = __ballot(head);
            if (lane == 0) {
                heads[c * 8u + wave * 2u] = (uint32_t)m;
                heads[c * 8u + wave * 2u + 1u] = (uint32_t)(m >> 32);
            }
        }
        __syncthreads();
        const uint64_t head_words = __ballot(heads[lane] != 0);
        // ---- run by run (the same runs in every lane)
        uint32_t s = 0;
        while (s < vend) {
            uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)kid_shared_next_head(heads, head_words, s + 1u));
            if (e > vend) e = vend;
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)targ[s]);
            if (t != cur_t) {
                flush();
                cur_t = t;
            }
            const uint32_t q_begin = s >> 7, q_end = (e + 127u) >> 7;
            for (uint32_t q = q_begin + ((sub - q_begin) & (split - 1u)); q < q_end; q += split) {
                const uint32_t lo = q << 7;
                uint4 m = make_uint4(~0u, ~0u, ~0u, ~0u);
                if (lo < s || lo + 128u > e) // a quad the run does not cover
                    m = make_uint4(kid_shared_word_mask(s, e, lo), kid_shared_word_mask(s, e, lo + 32u), kid_shared_word_mask(s, e, lo + 64u),
                                   kid_shared_word_mask(s, e, lo + 96u));
#pragma unroll
                for (int k = 0; k < KID_SHARED_SLOTS; k++) {
                    if (pij[k] == ~0u) continue;
                    const uint4 x = *reinterpret_cast<const uint4 *>(&bits[(pij[k] & 255u) * KID_SHARED_ROW + q * 4u]);
                    const uint4 y = *reinterpret_cast<const uint4 *>(&bits[(pij[k] >> 8) * KID_SHARED_ROW + q * 4u]);
                    acc[k] += (uint32_t)(__popc(x.x & y.x & m.x) + __popc(x.y & y.y & m.y) + __popc(x.z & y.z & m.z) + __popc(x.w & y.w & m.w));
                }
            }
            s = e;
        }
        __syncthreads();
    }
    flush();
}

// shared[j][i][t] = shared[i][j][t] for i < j
__global__ void kid_shared_mirror_kernel(unsigned long long *shared, uint32_t n, uint32_t ntar)
{
    const uint64_t total = (uint64_t)n * n * ntar;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)(x % ntar);
        const uint32_t ij = (uint32_t)(x / ntar), i = ij / n, j = ij % n;
        if (i > j) shared[x] = shared[((uint64_t)j * n + i) * ntar + t];
    }
}
