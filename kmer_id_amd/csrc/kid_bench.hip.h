// kid_bench.hip.h -- kernels no classification runs: the synthetic workload and the random-gather ceiling (kid_api_bench.h).
#pragma once
#include "kid_kernels.hip.h"

// ------------------------------------------------------------------ synthetic data
__global__ void kid_synth_keys_kernel(uint64_t seed, int k, const uint64_t *cum, int32_t ntar, uint64_t j0, uint64_t n,
                                      uint64_t *keys, uint32_t *targets)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        keys[i] = kid_synth_db_key(seed, k, j0 + i);
        targets[i] = kid_synth_target_of(cum, ntar, j0 + i);
    }
}

__global__ void kid_synth_reads_kernel(uint64_t db_seed, uint64_t read_seed, int k, const uint64_t *cum,
                                       const int32_t *parent, int32_t ntar, uint64_t r0, uint64_t n, uint32_t len,
                                       uint8_t *bases)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        kid_synth_read(db_seed, read_seed, k, cum, parent, ntar, r0 + i, len, bases + i * (uint64_t)len);
}

// ------------------------------------------------------------------ random-gather ceiling
// INF independent 16-byte loads per lane per round from uniformly random cells
// The same question asked the way the classify kernel asks it: random 128-byte LINES of the table (cell 0 of a line),
// RUN consecutive lanes on one line (1: 64 distinct lines per load; 8: what the headers of neighbouring k-mers look like),
// four loads in flight per lane, issued from inline assembly and waited for once.
template <int RUN, int MODE = 0> // MODE bit 0: a random cell of the line instead of cell 0; bit 1: the compiler's load and wait instead of inline assembly
__global__ __launch_bounds__(256) void kid_gather_lines_kernel(const uint4 *table, uint32_t line_mask, uint64_t rounds, uint32_t *sink)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    uint32_t acc = 0;
    uint64_t ctr = wave * 0x9E3779B97F4A7C15ULL + 12345;
    for (uint64_t r = 0; r < rounds; r++) {
        kid_u4 a[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ctr += 0xD1B54A32D192ED03ULL;
            const uint32_t line = (uint32_t)kid_fmix64(ctr ^ ((uint64_t)(lane / (uint32_t)RUN) << 48)) & line_mask;
            const uint4 *p = table + (uint64_t)line * KID_LINE_CELLS + ((MODE & 1) ? (uint32_t)(ctr >> 40) & 7u : 0u);
            if (MODE & 2) { const uint4 v = *p; a[u] = kid_u4{v.x, v.y, v.z, v.w}; }
            else asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(a[u]) : "v"(p) : "memory");
        }
        if (!(MODE & 2)) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : : "memory");
#pragma unroll
        for (int u = 0; u < 4; u++) acc ^= a[u].x ^ a[u].z;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

// ... and of the digest plane (kid_common.h): the same random lines, the same runs, one 8-byte load per lane from the
// line's digest instead of 16 bytes from its header
template <int RUN>
__global__ __launch_bounds__(256) void kid_gather_digest_kernel(const uint2 *digest, uint32_t line_mask, uint64_t rounds, uint32_t *sink)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    uint32_t acc = 0;
    uint64_t ctr = wave * 0x9E3779B97F4A7C15ULL + 12345;
    for (uint64_t r = 0; r < rounds; r++) {
        kid_u2 a[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ctr += 0xD1B54A32D192ED03ULL;
            const uint32_t line = (uint32_t)kid_fmix64(ctr ^ ((uint64_t)(lane / (uint32_t)RUN) << 48)) & line_mask;
            const uint2 *p = digest + line;
            asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(a[u]) : "v"(p) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : : "memory");
#pragma unroll
        for (int u = 0; u < 4; u++) acc ^= a[u].x ^ a[u].y;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

template <int INF>
__global__ __launch_bounds__(256) void kid_gather_kernel(const uint4 *table, uint32_t slot_mask, uint64_t rounds, uint32_t *sink)
{
    const uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint32_t acc = 0;
    uint64_t ctr = tid * 0x9E3779B97F4A7C15ULL;
    for (uint64_t r = 0; r < rounds; r++) {
        uint4 c[INF];
#pragma unroll
        for (int u = 0; u < INF; u++) {
            ctr += 0xD1B54A32D192ED03ULL;
            c[u] = table[(uint32_t)kid_fmix64(ctr) & slot_mask];
        }
#pragma unroll
        for (int u = 0; u < INF; u++) acc ^= c[u].x ^ c[u].z;
    }
    if (acc == 0x12345678u) sink[0] = acc; // never true in practice; keeps the loads alive
}
