// kid_seenlog.hip.h -- the hit log of the classify kernels -> seen-bitmap, and the bitmap -> ucount.
#pragma once
#include "kid_table.hip.h"

#define KID_LOG_SHARDS 64u      // regions (blockIdx & 63), each with its own fill counter: a resolver chunk costs one fetch-and-add on
                                // its region's counter, and with 16 hits per read (reads from genomes the database holds) there are
                                // 600 k chunks per 1 M pairs -- on 8 counters they queued for 3 ms (profiles/r03/clumped_db_log_shards.txt)
#define KID_LOG_NONE 0xFFFFFFFFu // a log place whose lookup turned out not to be a hit
#define KID_LOG_BIN_BITS 18     // the apply pass owns the bitmap in pieces of 2^18 bits = 32 KiB of LDS
#define KID_LOG_WGS 1024u       // workgroups of the counting / scattering kernels: 16 per region

// ------------------------------------------------------------------ the hit log -> seen-bitmap
// The classify kernels append the entry ordinals of their hits to KID_LOG_SHARDS log regions.  Setting 2.5 M random
// bits of a 13.6 MB bitmap costs one memory-side atomic each however it is done from the classify kernel; here the
// entries are first sorted by bitmap piece (a counting sort: count, scan, scatter), then ONE workgroup per piece sets
// its bits in LDS and ORs the piece into the bitmap as its only writer.  Run every few dozen launches (and before
// anybody reads the bitmap), over everything logged since: ~16 bytes of traffic per logged hit + one pass over the bitmap.
struct KidLogArgs {
    const uint32_t *log;
    const uint32_t *tail;
    uint32_t cap;
    uint32_t nbins;        // pieces of 2^KID_LOG_BIN_BITS bits
    uint32_t *counts;      // [bin][workgroup]: entries of the bin in the workgroup's share of the log
    uint32_t *bin_total;   // [bin]
    uint32_t *sorted;
    uint32_t *seen;
    uint64_t seen_words;
    unsigned long long *host_total; // mapped host memory: log places asked for per 1024 reads, as of this pass (the host paces the passes by it)
    // Many hits per read (reads from genomes the database holds): neighbouring lookups name neighbouring bits, the
    // resolver merges them over DPP and one atomic sets up to 16 -- cheaper than logging every hit and sorting the log
    // (profiles/r03/dense_hits.txt: 15 hits per read 1-2 %, 60 hits 4.5 %, the builder-shaped database 6 %).  The
    // pass decides: more than 8 log places per read of the `reads` it covers, and it takes the log out of the sample's
    // argument blocks -- in stream order, in front of the next launch, without a trip to the host.
    unsigned long long reads;
    KidRareArgs *blocks[4];
    unsigned int *off_flag;         // mapped host memory: set when the pass has switched the log off
};
// the share of the log a counting / scattering workgroup owns: region blockIdx / 16, 1/16 of its entries (whole
// groups of 64 entries: a share starts on a 16-byte boundary)
__device__ __forceinline__ void kid_log_share(const KidLogArgs &a, uint32_t &begin, uint32_t &end)
{
    const uint32_t per = KID_LOG_WGS / KID_LOG_SHARDS, sh = blockIdx.x / per, c = blockIdx.x % per;
    const uint32_t t = a.tail[sh * 16u], filled = t < a.cap ? t : a.cap;
    const uint32_t len = ((filled + per - 1u) / per + 63u) & ~63u;
    begin = sh * a.cap + (c * len < filled ? c * len : filled);
    end = sh * a.cap + ((c + 1u) * len < filled ? (c + 1u) * len : filled);
}
// every entry of [b0, b1) to f, four at a time (16-byte loads: these kernels are a stream over the log)
template <class F>
__device__ __forceinline__ void kid_log_for_each(const uint32_t *log, uint32_t b0, uint32_t b1, F &&f)
{
    const uint32_t n4 = (b1 - b0) >> 2;
    const uint4 *p = reinterpret_cast<const uint4 *>(log + b0);
    for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) {
        const uint4 v = p[i];
        if (v.x != KID_LOG_NONE) f(v.x);
        if (v.y != KID_LOG_NONE) f(v.y);
        if (v.z != KID_LOG_NONE) f(v.z);
        if (v.w != KID_LOG_NONE) f(v.w);
    }
    for (uint32_t i = b0 + (n4 << 2) + threadIdx.x; i < b1; i += blockDim.x) {
        const uint32_t e = log[i];
        if (e != KID_LOG_NONE) f(e);
    }
}
__global__ __launch_bounds__(256) void kid_seenlog_count_kernel(const KidLogArgs a)
{
    extern __shared__ uint32_t kid_lh[];
    for (uint32_t i = threadIdx.x; i < a.nbins; i += blockDim.x) kid_lh[i] = 0;
    __syncthreads();
    uint32_t b0, b1;
    kid_log_share(a, b0, b1);
    kid_log_for_each(a.log, b0, b1, [&](const uint32_t e) { atomicAdd(&kid_lh[e >> KID_LOG_BIN_BITS], 1u); });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.nbins; i += blockDim.x) a.counts[i * KID_LOG_WGS + blockIdx.x] = kid_lh[i];
}
// per bin: exclusive scan of the workgroups' counts (in place) and the bin's total
__global__ __launch_bounds__(1024) void kid_seenlog_scan_kernel(const KidLogArgs a)
{
    __shared__ uint32_t part[KID_LOG_WGS];
    uint32_t *c = a.counts + (size_t)blockIdx.x * KID_LOG_WGS;
    const uint32_t v = c[threadIdx.x];
    part[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 1; o < KID_LOG_WGS; o <<= 1) {
        const uint32_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    c[threadIdx.x] = part[threadIdx.x] - v;
    if (threadIdx.x == KID_LOG_WGS - 1u) a.bin_total[blockIdx.x] = part[threadIdx.x];
}
// inclusive scan over the 64 lanes of a wave
template <class T>
__device__ __forceinline__ T kid_wave_incscan(T x)
{
    using S = typename std::conditional<sizeof(T) == 8, unsigned long long, int>::type; // (what __shfl_up moves)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = (T)__shfl_up((S)x, (unsigned)o);
        if ((int)(threadIdx.x & 63u) >= o) x += y;
    }
    return x;
}
// Exclusive scan over the 4 x 256 values of a workgroup of 256 threads, thread t holding values 4t .. 4t + 3 in x[]:
// x[j] becomes the sum of everything before it; returns the sum up to and including the thread's own (thread 255: the
// total).  wave_tot: LDS [4], the waves' totals afterwards; the caller's barrier comes before it is written again.
template <class T>
__device__ __forceinline__ T kid_block_exscan4(T (&x)[4], T *wave_tot)
{
    const uint32_t wv = threadIdx.x >> 6;
    const T sum = x[0] + x[1] + x[2] + x[3], inc = kid_wave_incscan(sum);
    if ((threadIdx.x & 63u) == 63u) wave_tot[wv] = inc;
    __syncthreads();
    T run = inc - sum;
    for (uint32_t w = 0; w < wv; w++) run += wave_tot[w];
#pragma unroll
    for (int j = 0; j < 4; j++) { const T v = x[j]; x[j] = run; run += v; }
    return run;
}
// where the bins start in `sorted`: exclusive scan of bin_total (<= 1024 bins) into LDS; returns the grand total
__device__ __forceinline__ uint32_t kid_log_bin_bases(const KidLogArgs &a, uint32_t *bases /* nbins + 1 */)
{
    // (one wave does it: the totals are few)
    if (threadIdx.x < 64u) {
        uint32_t run = 0;
        for (uint32_t i0 = 0; i0 < a.nbins; i0 += 64u) {
            const uint32_t i = i0 + threadIdx.x;
            const uint32_t v = i < a.nbins ? a.bin_total[i] : 0u, x = kid_wave_incscan(v);
            if (i < a.nbins) bases[i] = run + x - v;
            run += (uint32_t)__shfl((int)x, 63);
        }
        if (threadIdx.x == 0) bases[a.nbins] = run;
    }
    __syncthreads();
    return bases[a.nbins];
}
// exclusive scan of v[0 .. n) (n <= 4 x blockDim) into out[0 .. n), by a workgroup of 256 threads; returns the total
__device__ __forceinline__ uint32_t kid_block_exscan(const uint32_t *v, uint32_t *out, const uint32_t n, uint32_t *wave_tot /* [5] */)
{
    const uint32_t i0 = 4u * threadIdx.x;
    uint32_t x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = i0 + j < n ? v[i0 + j] : 0u;
    kid_block_exscan4(x, wave_tot);
#pragma unroll
    for (int j = 0; j < 4; j++) if (i0 + j < n) out[i0 + j] = x[j];
    const uint32_t total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    return total;
}
// The log -> `sorted`, bin by bin.  A workgroup takes its share in tiles of KID_LOG_TILE entries and sorts a tile in LDS
// first (count, scan, place), so that what goes out to memory are runs of neighbouring entries of one bin -- scattering
// the entries one by one took 7 ps each (47 M partial-line writes per pass, profiles/r03/seen_log_first_kernel_stats.csv).
#define KID_LOG_TILE 4096u
__global__ __launch_bounds__(256) void kid_seenlog_scatter_kernel(const KidLogArgs a)
{
    extern __shared__ uint32_t kid_lh[]; // bin bases [nbins + 1], next place of this workgroup per bin [nbins], the tile's counts and offsets [2 nbins], the tile
    const uint32_t nb = a.nbins;
    uint32_t *bases = kid_lh, *next = bases + nb + 1u, *hist = next + nb, *toff = hist + nb, *stage = toff + nb;
    __shared__ uint32_t wave_tot[5];
    kid_log_bin_bases(a, bases);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // (by the places ASKED for -- hits, header matches that were none, and what no longer fitted: a log that
        // overflows holds fewer entries than there were hits.  Reported as ONE word, a rate: the host runs far ahead of
        // the device, and a count would meet the wrong number of reads there)
        unsigned long long asked = 0;
        for (uint32_t i = 0; i < KID_LOG_SHARDS; i++) asked += a.tail[i * 16u];
        if (a.host_total && a.reads) *a.host_total = ((asked << 10) / a.reads) | (1ull << 63);
        if (a.reads && asked > 8ull * a.reads) {
            for (int i = 0; i < 4; i++)
                if (a.blocks[i]) a.blocks[i]->seen_log = nullptr;
            if (a.off_flag) *a.off_flag = 1u;
        }
    }
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) next[i] = bases[i] + a.counts[i * KID_LOG_WGS + blockIdx.x];
    uint32_t b0, b1;
    kid_log_share(a, b0, b1);
    for (uint32_t t0 = b0; t0 < b1; t0 += KID_LOG_TILE) { // (workgroup-uniform)
        const uint32_t n = b1 - t0 < KID_LOG_TILE ? b1 - t0 : KID_LOG_TILE;
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        uint32_t e[KID_LOG_TILE / 256u], r[KID_LOG_TILE / 256u];
#pragma unroll
        for (uint32_t j = 0; j < KID_LOG_TILE / 256u; j++) {
            const uint32_t i = j * 256u + threadIdx.x;
            e[j] = i < n ? a.log[t0 + i] : KID_LOG_NONE;
        }
#pragma unroll
        for (uint32_t j = 0; j < KID_LOG_TILE / 256u; j++)
            r[j] = e[j] != KID_LOG_NONE ? atomicAdd(&hist[e[j] >> KID_LOG_BIN_BITS], 1u) : 0u; // its rank among the tile's entries of its bin
        __syncthreads();
        const uint32_t tile_n = kid_block_exscan(hist, toff, nb, wave_tot);
#pragma unroll
        for (uint32_t j = 0; j < KID_LOG_TILE / 256u; j++)
            if (e[j] != KID_LOG_NONE) stage[toff[e[j] >> KID_LOG_BIN_BITS] + r[j]] = e[j];
        __syncthreads();
        for (uint32_t p = threadIdx.x; p < tile_n; p += blockDim.x) { // neighbours in `stage` are neighbours in `sorted`
            const uint32_t v = stage[p], bin = v >> KID_LOG_BIN_BITS;
            a.sorted[next[bin] + (p - toff[bin])] = v;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) next[i] += hist[i];
        __syncthreads();
    }
}
__global__ __launch_bounds__(1024) void kid_seenlog_apply_kernel(const KidLogArgs a)
{
    extern __shared__ uint32_t kid_lh[]; // 2^KID_LOG_BIN_BITS bits of the bitmap, then the bin bases
    const uint32_t piece_words = 1u << (KID_LOG_BIN_BITS - 5);
    uint32_t *piece = kid_lh, *bases = kid_lh + piece_words;
    kid_log_bin_bases(a, bases);
    const uint32_t e0 = bases[blockIdx.x], e1 = bases[blockIdx.x + 1u];
    if (e0 == e1) return; // (workgroup-uniform)
    for (uint32_t i = threadIdx.x; i < piece_words; i += blockDim.x) piece[i] = 0;
    __syncthreads();
    auto set = [&](const uint32_t v) { const uint32_t e = v & ((1u << KID_LOG_BIN_BITS) - 1u); atomicOr(&piece[e >> 5], 1u << (e & 31u)); };
    // the bin's entries, 16 bytes per load between the first and the last 16-byte boundary
    const uint32_t up = (e0 + 3u) & ~3u, a0 = up < e1 ? up : e1, a1 = a0 + ((e1 - a0) & ~3u);
    for (uint32_t i = e0 + threadIdx.x; i < a0; i += blockDim.x) set(a.sorted[i]);
    const uint4 *p4 = reinterpret_cast<const uint4 *>(a.sorted + a0);
    for (uint32_t i = threadIdx.x; i < (a1 - a0) >> 2; i += blockDim.x) { const uint4 v = p4[i]; set(v.x); set(v.y); set(v.z); set(v.w); }
    for (uint32_t i = a1 + threadIdx.x; i < e1; i += blockDim.x) set(a.sorted[i]);
    __syncthreads();
    const uint64_t w0 = (uint64_t)blockIdx.x * piece_words;
    for (uint32_t i = threadIdx.x; i < piece_words; i += blockDim.x) {
        const uint32_t v = piece[i];
        if (v && w0 + i < a.seen_words) a.seen[w0 + i] |= v; // the only writer of this piece while the pass runs
    }
}

// ------------------------------------------------------------------ ucount from the seen-bitmap
// ucount[t] = number of distinct DB k-mers of target t seen in the sample
// (newkmer_10nx.cpp:596-603), counted over the entry ordinals [w_begin*32, w_end*32): bit o of the
// bitmap = "the key first inserted as entry o was hit", ord_target[o] = that entry's target
template <bool HIST>
__global__ void kid_ucount_kernel(const uint32_t *seen, uint64_t w_begin, uint64_t w_end, const uint32_t *ord_target,
                                  unsigned long long *ucount, uint32_t ntar)
{
    // the bitmap is almost empty: stream it 16 bytes per lane and only look inside non-zero words;
    // counts go to a per-workgroup LDS histogram first (millions of hits land on a few thousand targets)
    extern __shared__ uint32_t kid_uhist[];
    if (HIST) {
        for (uint32_t i = threadIdx.x; i < ntar; i += blockDim.x) kid_uhist[i] = 0;
        __syncthreads();
    }
    const uint64_t q_begin = w_begin >> 2, q_end = w_end >> 2; // callers pass 128-cell aligned ranges
    const uint4 *seen4 = reinterpret_cast<const uint4 *>(seen);
    for (uint64_t q = q_begin + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < q_end; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 v = seen4[q];
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t bits = words[i];
            while (bits) {
                const uint32_t bpos = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1;
                const uint32_t t = ord_target[(q * 4ull + (uint64_t)i) * 32ull + bpos];
                if (HIST) atomicAdd(&kid_uhist[t], 1u);
                else atomicAdd(&ucount[t], 1ull);
            }
        }
    }
    if (HIST) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < ntar; i += blockDim.x) {
            const uint32_t c = kid_uhist[i];
            if (c) atomicAdd(&ucount[i], (unsigned long long)c);
        }
    }
}

__global__ void kid_or_kernel(uint32_t *dst, const uint32_t *src, uint64_t nwords)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * blockDim.x)
        dst[i] |= src[i];
}
