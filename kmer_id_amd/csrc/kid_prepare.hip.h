// kid_prepare.hip.h -- ASCII bases -> 2-bit codes, and the kernels in front of a classify launch: read descriptors from
// [start, stop] or from FASTQ quality lines (process_qual), the launch's argument block.
#pragma once
#include "kid_table.hip.h"

// ------------------------------------------------------------------ base packing
// ASCII bases -> 2-bit codes plus a mask of the bytes that are not ACGTacgt (those reset the reference's
// rolling window, newkmer_10nx.cpp:520-524).  4 bytes at a time, no per-byte branches.
// kid_pack4: the 4 bases of one dword (byte 0 = first base) -> codes in bits 7:0 (first base in bits 7:6),
// invalid flags in bits 3:0 of inv (bit j = byte j).
__device__ __forceinline__ void kid_pack4(const uint32_t x, const uint32_t u_is_t, uint32_t &codes, uint32_t &inv)
{
    const uint32_t c = ((x >> 1) ^ (x >> 2)) & 0x03030303u; // A,C,G,T -> 0,1,2,3 in every byte
    codes = (c * 0x40100401u) >> 24;                        // byte0 -> bits 7:6 ... byte3 -> bits 1:0
    // rebuild the upper-case letter each code stands for and compare
    const uint32_t c0 = c & 0x01010101u, c1 = (c >> 1) & 0x01010101u, t = c0 & c1;
    const uint32_t expect = 0x40404040u | (0x01010101u ^ t) | ((c0 ^ c1) << 1) | (c1 << 2) | (t << 4);
    uint32_t diff = (x & 0xDFDFDFDFu) ^ expect;
    if (u_is_t) diff &= ~t; // 'U' = 'T' ^ 1 and decodes to code 3
    const uint32_t nz = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;
    inv = (((nz >> 7) * 0x00204081u) >> 21) & 0xFu;
}
// The same split in two for the pair loops, where almost no read has a base that is not ACGT: the codes and a word
// `diff` that is non-zero in every byte that is not ACGTacgt(Uu) -- seven instructions (v_perm_b32 looks up the
// letter a code stands for, v_dot4_u32_u8 gathers the four codes) --, and the 4-bit mask from `diff` when somebody
// needs it.
__device__ __forceinline__ uint32_t kid_codes4(const uint32_t x, const uint32_t u_is_t, uint32_t &diff)
{
    const uint32_t c = ((x >> 1) ^ (x >> 2)) & 0x03030303u;            // A,C,G,T -> 0,1,2,3 in every byte
    const uint32_t expect = __builtin_amdgcn_perm(0u, 0x54474341u, c); // byte j = "ACGT"[code of byte j]
    diff = (x & 0xDFDFDFDFu) ^ expect;
    if (u_is_t) diff &= ~(c & (c >> 1) & 0x01010101u);                 // 'U' = 'T' ^ 1 and decodes to code 3
    return __builtin_amdgcn_udot4(c, 0x01041040u, 0u, false);          // byte0 -> bits 7:6 ... byte3 -> bits 1:0
}
__device__ __forceinline__ uint32_t kid_inv4(const uint32_t diff)
{
    const uint32_t nz = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;
    return (((nz >> 7) * 0x00204081u) >> 21) & 0xFu;
}
// 16 bases -> one packed word (first base in the top bits) + 16-bit mask
__device__ __forceinline__ void kid_pack16(const uint4 v, const uint32_t u_is_t, uint32_t &codes, uint32_t &inv)
{
    const uint32_t in[4] = {v.x, v.y, v.z, v.w};
    codes = 0;
    inv = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t c8, i4;
        kid_pack4(in[q], u_is_t, c8, i4);
        codes = (codes << 8) | c8;
        inv |= i4 << (4 * q);
    }
}

// ------------------------------------------------------------------ batch preparation
// What a launch of the classify kernels finds in its device argument block: its share of the descriptors (or the fixed
// layout) and of the result array.  Set in classify-stream order.
__device__ __forceinline__ void kid_rebase(KidRareArgs *rare, const KidReadDesc *desc, uint32_t *out_final, unsigned long long read0,
                                           uint32_t fixed_len, int32_t fixed_nk)
{
    if (threadIdx.x == 0) {
        rare->desc = desc;
        rare->out_final = out_final;
        rare->read0 = read0;
        rare->fixed_len = fixed_len;
        rare->fixed_nk = fixed_nk;
    }
}

// [start, stop] -> descriptor; the range checks the reference leaves to string::at() happen here
__global__ void kid_prepare_kernel(const KidBatch b, int k, KidReadDesc *desc, unsigned long long *stats, KidRareArgs *rare, uint32_t seq,
                                   uint32_t long_cut, KidLongList *long_list, int rebase)
{
    // (the launch's descriptor / result pointers are set in classify-stream order: by kid_rebase_kernel when this kernel
    //  may run while the batch before is being classified, else -- `rebase`, same stream -- right here for the batch's
    //  first launch: one launch and its gap less per batch)
    if (rebase && blockIdx.x == 0) kid_rebase(rare, desc, b.out_final, 0ull, 0u, 0);
    uint32_t bad = 0, mx = 0;
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < b.n; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t off;
        int64_t rl;
        if (b.offsets) { off = b.offsets[r]; rl = (int64_t)(b.offsets[r + 1] - off); }
        else { off = r * (uint64_t)b.fixed_len; rl = b.fixed_len; }
        int64_t s0 = b.start ? (int64_t)b.start[r] : 0;
        int64_t e0 = b.stop ? (int64_t)b.stop[r] : rl - 1;
        if (s0 <= e0 && (s0 < 0 || e0 >= rl)) { // never read outside the read; reported as KID_ERR_ARG
            bad++;
            if (s0 < 0) s0 = 0;
            if (e0 >= rl) e0 = rl - 1;
        }
        KidReadDesc d;
        int64_t nk = e0 - s0 + 1 - (k - 1);
        if (s0 > e0) nk = 0;
        d.first_base = off + (uint64_t)(s0 > 0 ? s0 : 0);
        d.n_kmers = (int32_t)(nk > 0x7FFFFFFF ? 0x7FFFFFFF : nk);
        d.pad = 0;
        // a record that goes to the long-record kernels (kid_long_hits_kernel / kid_long_fold_kernel): the classify
        // kernels see a read without k-mers (counted under target 0 until the fold corrects that)
        if (long_cut && nk > (int64_t)long_cut) {
            const uint32_t at = atomicAdd(&long_list->n, 1u);
            if (at < KID_LONG_MAX) {
                KidLongList::Item it;
                it.first_base = d.first_base; it.n_kmers = (uint32_t)d.n_kmers; it.read = (uint32_t)r;
                long_list->e[at] = it;
                d.n_kmers = 0;
            }
        }
        desc[r] = d;
        if (d.n_kmers > 0 && (uint32_t)d.n_kmers > mx) mx = (uint32_t)d.n_kmers;
    }
    // largest read of the batch, tagged with the batch number so that the word never needs a reset: one
    // atomic per workgroup at most (none once a workgroup sees a value as large as its own; a batch of
    // equal reads is announced by workgroup 0 alone)
    __shared__ uint32_t s_mx;
    if (threadIdx.x == 0) s_mx = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)mx, o); mx = y > mx ? y : mx; }
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&s_mx, mx);
    __syncthreads();
    const bool uniform_batch = !b.offsets && !b.start && !b.stop;
    if (threadIdx.x == 0 && (!uniform_batch || blockIdx.x == 0)) {
        const unsigned long long v = ((unsigned long long)seq << 32) | s_mx;
        if (v > *reinterpret_cast<volatile unsigned long long *>(&rare->batch_max)) atomicMax(&rare->batch_max, v);
    }
    if (bad) atomicAdd(&stats[4], (unsigned long long)bad);
}

// Sets a launch's argument block without kid_prepare_kernel: the later launches of a batch classified in several, and
// every launch of a fixed-layout batch (no descriptors: the host knows the one read length; batch_max = (seq << 32) | k-mers)
__global__ void kid_rebase_kernel(KidRareArgs *rare, const KidReadDesc *desc, uint32_t *out_final, unsigned long long read0,
                                  uint32_t fixed_len, int32_t fixed_nk, unsigned long long batch_max)
{
    kid_rebase(rare, desc, out_final, read0, fixed_len, fixed_nk);
    if (threadIdx.x == 0 && batch_max) rare->batch_max = batch_max;
}

// process_qual, newkmer_10nx.cpp:714-760: the quality string of one read (len = length of its SEQUENCE, :716) ->
// [start, stop].  A sequential scan by nature: one read per thread.
__device__ __forceinline__ void kid_process_qual(const signed char *q, const int len, int &start, int &stop)
{
    start = 0;
    stop = len - 1;
    if (len <= 0) return;
    while (q[start] < 49 && start < stop) start++;
    while (q[stop] < 49 && stop > start) stop--;
    if (start < stop - 4) {
        int w = 0;
        for (int i = 0; i < 4; i++) w += q[start + i] - 32;
        while (w < 68 && start < stop - 4) { w += q[start + 4] - q[start]; start++; }
    }
    if (start < stop - 4) {
        int w = 0;
        for (int i = 0; i < 4; i++) w += q[stop - i] - 32;
        while (w < 68 && start < stop - 4) { w += q[stop - 4] - q[stop]; stop--; }
    }
}

__global__ void kid_trim_kernel(const uint8_t *quals, const uint64_t *offsets, uint64_t n, int k,
                                int32_t *start_out, int32_t *stop_out, uint8_t *keep)
{
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const int len = (int)(offsets[r + 1] - offsets[r]);
        int start, stop;
        kid_process_qual(reinterpret_cast<const signed char *>(quals + offsets[r]), len, start, stop);
        start_out[r] = start;
        stop_out[r] = stop;
        keep[r] = (len > 0 && stop - start >= k) ? 1 : 0;
    }
}

// A block of FASTQ text whose lines the host has found (kid_classify_fastq_async): process_qual + the ">= k" test
// of :757 + the read descriptor, per record.  A record process_qual drops is not handed to process_read in the
// reference, i.e. it is counted nowhere: the classify kernels see it as a read without k-mers (gcount[0]++), which
// this kernel takes back (stats[5] counts them).  stats[8]: records whose quality line is shorter than the sequence
// (qual.at() throws, :727).
struct KidFastqRec {
    uint32_t seq_off, seq_len, qual_off, qual_len; // byte offsets into the block's text
};
__global__ void kid_prepare_fastq_kernel(const uint8_t *text, const KidFastqRec *recs, uint64_t n, int k, KidReadDesc *desc,
                                         int32_t *start_out, int32_t *stop_out, uint32_t *out_final, unsigned long long *stats,
                                         unsigned long long *gcount, KidRareArgs *rare, uint32_t seq, int rebase)
{
    if (rebase && blockIdx.x == 0) kid_rebase(rare, desc, out_final, 0ull, 0u, 0);
    uint32_t mx = 0, dropped = 0, bad = 0;
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const KidFastqRec rc = recs[r];
        int start = 0, stop = -1;
        if (rc.qual_len < rc.seq_len) bad++;
        else kid_process_qual(reinterpret_cast<const signed char *>(text + rc.qual_off), (int)rc.seq_len, start, stop);
        const bool keep = rc.seq_len > 0 && rc.qual_len >= rc.seq_len && stop - start >= k;
        KidReadDesc d;
        d.first_base = (uint64_t)rc.seq_off + (uint64_t)(start > 0 ? start : 0);
        d.n_kmers = keep ? stop - start + 1 - (k - 1) : 0;
        d.pad = 0;
        desc[r] = d;
        start_out[r] = start;
        stop_out[r] = stop;
        if (!keep) dropped++;
        if (d.n_kmers > 0 && (uint32_t)d.n_kmers > mx) mx = (uint32_t)d.n_kmers;
    }
    __shared__ uint32_t s_mx, s_dropped, s_bad;
    if (threadIdx.x == 0) { s_mx = 0; s_dropped = 0; s_bad = 0; }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)mx, o);
        mx = y > mx ? y : mx;
        dropped += (uint32_t)__shfl_xor((int)dropped, o);
        bad += (uint32_t)__shfl_xor((int)bad, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (mx) atomicMax(&s_mx, mx);
        if (dropped) atomicAdd(&s_dropped, dropped);
        if (bad) atomicAdd(&s_bad, bad);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long v = ((unsigned long long)seq << 32) | s_mx;
        if (v > *reinterpret_cast<volatile unsigned long long *>(&rare->batch_max)) atomicMax(&rare->batch_max, v);
        if (s_dropped) { atomicAdd(&gcount[0], 0ull - (unsigned long long)s_dropped); atomicAdd(&stats[5], (unsigned long long)s_dropped); }
        if (s_bad) atomicAdd(&stats[8], (unsigned long long)s_bad);
    }
}
