// kid_lowc.hip.h -- mask low-complexity sequence: a fixed-window, symmetric form of the DUST score.  Every base whose
// window of 64 positions is dominated by a few repeated triplets becomes 'N' in the DEVICE copy of the text, in front of
// the unchanged kernels that read it (the quality mask, kid_mask.hip.h, is its elder sibling).
//
// The rule.  A line is one read's whole sequence s[0, len).  A byte is a base when the lookup takes it as one
// (ACGTacgt, Uu under KID_FLAG_U_IS_T); triplet i is valid when bytes i, i + 1, i + 2 are bases of the line, and its
// value is made of their three 2-bit codes.  The window of position p holds the valid triplets that lie inside
// [max(0, p - 32), min(len, p + 32)); l is their number, c_v how many have value v, S = sum c_v (c_v - 1) / 2.
// p is low when l >= 2 and 10 S > T (l - 1); every low position that holds a base becomes 'N'.  All decisions of a line
// are taken on the text as it was before this mask wrote anything.
// (The clipping of the window is the same as reading every byte outside the line as no base: the triplets of p are then
// simply i = p - 32 .. p + 29.  S depends on which triplets are EQUAL alone, so any one-to-one code of the bases will do:
// here A, C, T/U, G = 0, 1, 2, 3, bits 1..2 of the ASCII byte.)
//
// The work.  One lane slides along one line, or along one CHUNK of a line that is longer than KID_LOWC_CHUNK.  It reads
// the text in aligned 16-byte groups (one 16-byte load: an aligned group that holds one byte of the line lies in that
// byte's page; bytes of the group outside the line, or in front of the chunk's halo, are read as no base and never
// used), turns a group into 16 codes and 16 "is a base" bits, and keeps the last four groups that way in registers: the
// triplet that LEAVES the window is taken from those, 64 bytes behind the one that enters, so the text is read once and
// a lane never reads a byte again that it has decided.  Step s (byte s of the line arrives) adds triplet s - 4,
// removes triplet s - 66 and decides position p = s - 33: two counter updates and an incremental S and l per base.  The
// 64 one-byte counters (a window holds at most 62 triplets) are in LDS, lane-interleaved -- counter v of lane t is byte
// v & 3 of dword (v >> 2) * 256 + t, so the lanes of a wave never share a bank: 16 KiB per workgroup of 256.
//
// Two passes where a line is split, one where it is not.  A chunk's lane reads 32 bytes (and the two more of the last
// triplet) on either side of its positions, which are positions another lane decides and would overwrite: so when any
// line of a batch is longer than KID_LOWC_CHUNK, the lanes write their decisions to a flag PLANE (one byte per byte of
// text, zeroed in front of the kernel; a byte store per masked base) and kid_lowc_apply_kernel stores the 'N's behind
// it.  A line that one lane owns from its first byte to its last has no such neighbour -- no other lane uses a byte of
// it -- and the lane has read what it is about to overwrite 33 bytes ago: it stores 'N' directly and there is no plane
// and no second kernel (the short-read case: nothing is allocated).  The decisions are the same in both forms and for
// every chunk size and grid: they are a function of the line alone.
// Either way: one BYTE store per masked base, no read-modify-write of text words, no byte outside a line's sequence
// written, and no atomic but the one add per workgroup to *n_masked (nullable).
//
// Lanes: work item w = (line w / parts, chunks w % parts, + parts, ..); parts = 1 unless the batch is split, so that
// consecutive lanes take consecutive chunks of a long record and a 1 Mb contig is spread over many waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kid_kernels.hip.h"

#define KID_LOWC_WINDOW 64
#define KID_LOWC_HALF 32
#define KID_LOWC_CHUNK 512u // positions a lane decides of a line that is split
#define KID_LOWC_BLOCK 256u
#define KID_LOWC_MAX_PARTS 256u

// bit (c & 0xDF) - 'A' of this word says that byte c is a base
#define KID_LOWC_BASE_BITS(u_is_t) ((1u << 0) | (1u << 2) | (1u << 6) | (1u << 19) | ((u_is_t) ? 1u << 20 : 0u))

// 16 bytes of text -> codes (2 bits each, byte j at bits 2j) and "is a base" (bit j)
__device__ __forceinline__ void kid_lowc_pack16(const uint4 v, const uint32_t base_bits, uint32_t &codes, uint32_t &bases)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    codes = 0;
    bases = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        // bits 1..2 of every byte, squeezed to one byte per word
        const uint32_t c = (w[q] >> 1) & 0x03030303u, t = c | (c >> 6);
        codes |= ((t & 0xFu) | ((t >> 12) & 0xF0u)) << (8 * q);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t y = ((w[q] >> (8 * j)) & 0xDFu) - 0x41u;
            bases |= (y < 32u ? (base_bits >> y) & 1u : 0u) << (4 * q + j);
        }
    }
}

// One lane: decides the positions [p0, p1) of the line at `line` (length len; p1 <= len), 'N' or flag `mark` to
// out[p] for every low base.  cnt: this lane's column of the counters.  -> bases masked
__device__ __forceinline__ uint32_t kid_lowc_span(const uint8_t *line, uint64_t len, uint64_t p0, uint64_t p1, uint32_t T,
                                                  uint32_t base_bits, uint8_t *out, uint8_t mark, uint8_t *cnt)
{
#pragma unroll
    for (int i = 0; i < 16; i++) *reinterpret_cast<uint32_t *>(cnt + i * (KID_LOWC_BLOCK * 4)) = 0;
    const int64_t n = (int64_t)len;
    const int64_t vb = p0 > KID_LOWC_HALF ? (int64_t)p0 - KID_LOWC_HALF : 0; // the first byte this lane takes as part of the line
    const int64_t s_end = (int64_t)p1 + KID_LOWC_HALF;                        // the step that decides p1 - 1
    const intptr_t a0 = (intptr_t)line;
    uint32_t gc1 = 0, gc2 = 0, gc3 = 0, gc4 = 0, gv1 = 0, gv2 = 0, gv3 = 0, gv4 = 0; // the groups 1..4 steps of 16 back
    uint32_t hc = 0, hv = 0, tc = 0, tv = 0; // the last codes / base bits of the entering and of the leaving side
    uint32_t S = 0, l = 0, masked = 0;
    for (intptr_t ga = (a0 + vb) & ~(intptr_t)15; (int64_t)(ga - a0) <= s_end; ga += 16) {
        const int64_t s0 = (int64_t)(ga - a0); // the step of the group's byte 0: -15 .. s_end
        uint32_t gc0 = 0, gv0 = 0;
        if (s0 < n) { // (s0 + 16 > vb always: the first group holds byte vb)
            kid_lowc_pack16(*reinterpret_cast<const uint4 *>(ga), base_bits, gc0, gv0);
            if (s0 < vb) gv0 &= 0xFFFFu << (uint32_t)(vb - s0);
            if (s0 + 16 > n) gv0 &= 0xFFFFu >> (uint32_t)(s0 + 16 - n);
        }
        // bit j: step s0 + j decides a position of [p0, p1) that holds a base (position s0 + j - 33: byte j - 1 of group 2)
        uint32_t dec = ((gv2 << 1) | (gv3 >> 15)) & 0xFFFFu;
        const int64_t j0 = (int64_t)p0 + KID_LOWC_HALF + 1 - s0, j1 = (int64_t)p1 + KID_LOWC_HALF + 1 - s0;
        if (j0 > 0) dec = j0 < 16 ? dec & (0xFFFFu << (uint32_t)j0) : 0u;
        if (j1 < 16) dec = j1 > 0 ? dec & (0xFFFFu >> (uint32_t)(16 - j1)) : 0u;
        uint8_t *const o = out + (s0 - (KID_LOWC_HALF + 1));
#pragma unroll
        for (int j = 0; j < 16; j++) {
            hc = (hc << 2) | ((gc0 >> (2 * j)) & 3u);
            hv = (hv << 1) | ((gv0 >> j) & 1u);
            tc = (tc << 2) | ((gc4 >> (2 * j)) & 3u);
            tv = (tv << 1) | ((gv4 >> j) & 1u);
            if (((hv >> 2) & 7u) == 7u) { // triplet s - 4 enters
                uint8_t *c = cnt + ((hc >> 6) & 15u) * (KID_LOWC_BLOCK * 4) + ((hc >> 4) & 3u);
                const uint32_t k = *c;
                S += k;
                l++;
                *c = (uint8_t)(k + 1u);
            }
            if ((tv & 7u) == 7u) { // triplet s - 66 leaves
                uint8_t *c = cnt + ((tc >> 2) & 15u) * (KID_LOWC_BLOCK * 4) + (tc & 3u);
                const uint32_t k = *c - 1u;
                S -= k;
                l--;
                *c = (uint8_t)k;
            }
            if (((dec >> j) & 1u) && l >= 2u && 10u * S > T * (l - 1u)) {
                o[j] = mark;
                masked++;
            }
        }
        gc4 = gc3; gc3 = gc2; gc2 = gc1; gc1 = gc0;
        gv4 = gv3; gv3 = gv2; gv2 = gv1; gv1 = gv0;
    }
    return masked;
}

// RECS: the lines of a FASTQ block (KidFastqRec: seq_off, seq_len into text), else offsets[0 .. n] into text.
// PLANE: decisions go to flags[] (one byte per byte of text, zero on entry) for kid_lowc_apply_kernel; else 'N' goes
// to the text at once -- only when no line is split: parts = 1 and every line is one chunk, whatever its length.
template <bool RECS, bool PLANE>
__global__ __launch_bounds__(KID_LOWC_BLOCK) void kid_lowc_mark_kernel(uint8_t *text, const KidFastqRec *recs, const uint64_t *offsets,
                                                                        uint64_t n, uint32_t parts, uint32_t T, uint32_t base_bits,
                                                                        uint8_t *flags, unsigned long long *n_masked)
{
    __shared__ uint32_t s_count[16 * KID_LOWC_BLOCK];
    uint8_t *const cnt = reinterpret_cast<uint8_t *>(s_count) + threadIdx.x * 4u;
    const uint64_t items = n * parts, stride = (uint64_t)gridDim.x * KID_LOWC_BLOCK;
    uint32_t masked = 0;
    for (uint64_t w = blockIdx.x * (uint64_t)KID_LOWC_BLOCK + threadIdx.x; w < items; w += stride) {
        const uint64_t r = w / parts;
        uint64_t off, len;
        if (RECS) {
            const KidFastqRec rc = recs[r];
            off = rc.seq_off;
            len = rc.seq_len;
        } else {
            off = offsets[r];
            len = offsets[r + 1] - off;
        }
        if (!PLANE) {
            if (len) masked += kid_lowc_span(text + off, len, 0, len, T, base_bits, text + off, (uint8_t)'N', cnt);
            continue;
        }
        for (uint64_t p0 = (w % parts) * KID_LOWC_CHUNK; p0 < len; p0 += (uint64_t)parts * KID_LOWC_CHUNK) {
            const uint64_t p1 = p0 + KID_LOWC_CHUNK < len ? p0 + KID_LOWC_CHUNK : len;
            masked += kid_lowc_span(text + off, len, p0, p1, T, base_bits, flags + off, 1, cnt);
        }
    }
    if (!n_masked) return;
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long c = masked;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (unsigned long long)__shfl_xor((long long)c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(n_masked, s_sum);
}

// flags[i] != 0 -> text[i] = 'N', i < nbytes; flags has whole 16-byte groups.  The flags are read 16 at a time, the
// text is not read at all.
__global__ __launch_bounds__(KID_LOWC_BLOCK) void kid_lowc_apply_kernel(uint8_t *text, const uint8_t *flags, uint64_t nbytes)
{
    const uint64_t groups = (nbytes + 15) / 16, stride = (uint64_t)gridDim.x * KID_LOWC_BLOCK;
    for (uint64_t g = blockIdx.x * (uint64_t)KID_LOWC_BLOCK + threadIdx.x; g < groups; g += stride) {
        const uint4 f = reinterpret_cast<const uint4 *>(flags)[g];
        if (!(f.x | f.y | f.z | f.w)) continue;
        const uint32_t w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (((w[j / 4] >> (8 * (j % 4))) & 0xFFu) && g * 16 + j < nbytes) text[g * 16 + j] = (uint8_t)'N';
    }
}
