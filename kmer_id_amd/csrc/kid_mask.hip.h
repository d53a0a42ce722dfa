// kid_mask.hip.h -- mask low-quality bases: every sequence byte whose quality byte, read as signed char the way
// process_qual reads it (newkmer_10nx.cpp:714-760), is below T = Q + 33 becomes 'N' in the DEVICE copy of the text.
// 'N' is no base to any kernel behind it (classify, hits, long records): a masked base breaks its k-mer windows like any
// byte that is not ACGTacgt(Uu), and everything downstream runs unchanged on the masked text.
//
// One kernel, two record sources:
//   RECS  a FASTQ block with the host's line index (KidFastqRec: seq_off / qual_off into one text).  A record with
//         qual_len < seq_len is skipped (it makes the batch KID_ERR_FORMAT anyway); quality bytes beyond seq_len are ignored.
//   else  bases + quals + offsets, qualities laid out like bases (as for kid_trim_kernel).  Reads lie back to back, and
//         base i is masked by quality byte i whatever read it belongs to: the batch is ONE span, offsets[0] .. offsets[n].
//
// The work: the kernel never reads the sequence, only the qualities.  A lane takes one ALIGNED 16-byte group of quality
// bytes (one 16-byte load: an aligned group that holds one byte of the span lies in that byte's page, so bytes of the
// group outside the span may be loaded -- they are masked out of the decision, never used), finds the bytes below T with
// three integer operations per word, and stores 'N' with one BYTE store per masked base.  So the alignment of the
// sequence never matters and that of the qualities only decides which lanes of the first and last group are partial:
// every combination of the two mod 16 takes the same path.  No word is read-modify-written: a dword shared by two reads
// (reads lie back to back) is never loaded from the sequence side at all.  No byte outside a record's sequence is
// written: a store happens only for an index i in [0, seq_len).  The decision depends on quality bytes alone, which no
// lane writes as long as no sequence line overlaps a quality line (the host checks the order of a FASTQ block's lines).
//
// Lanes of a TEAM of 16 take consecutive groups, i.e. 256 consecutive bytes of a record per step (a 150-base read is one
// step of 10 or 11 lanes; a wave holds four teams).  RECS: team t of the grid's x dimension takes records t, t + teams,
// ..; blockIdx.y splits every record once more, part y of gridDim.y taking the steps y, y + gridDim.y, .. (the host
// sizes gridDim.y from the longest record: 1 for short reads, so that a 1 Mb record is spread over many waves).  The
// other source is one span that all teams of the grid stride through.
// The number of bytes masked goes to *n_masked (nullable): lanes count, waves and the workgroup reduce, ONE atomic per
// workgroup that masked anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kid_kernels.hip.h"

#define KID_MASK_TEAM 16u                      // lanes per record
#define KID_MASK_STEP (KID_MASK_TEAM * 16u)    // quality bytes a team takes per step
#define KID_MASK_BLOCK 256u

// bit 7 of every byte of w that is, as a signed char, below t (34 <= t <= 126): bytes >= 128, and bytes < t.
// (w | 0x80..) - t * 0x01.. never borrows across bytes (every byte is >= 128 > t) and leaves bit 7 clear iff (b & 127) < t.
__device__ __forceinline__ uint32_t kid_mask_below(uint32_t w, uint32_t t_ones)
{
    return (~((w | 0x80808080u) - t_ones) | w) & 0x80808080u;
}
// bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ uint32_t kid_mask_pack4(uint32_t m) { return (((m >> 7) * 0x01020408u) >> 24) & 0xFu; }

// The share of one team in one span: seq[0, len) masked by qual[0, len).  part / parts: the steps this team takes.
// -> bases masked by this lane
__device__ __forceinline__ uint32_t kid_mask_span(uint8_t *seq, const uint8_t *qual, uint64_t len, uint64_t part, uint64_t parts,
                                                  uint32_t lane, uint32_t t_ones)
{
    if (len == 0) return 0;
    const uintptr_t q0 = (uintptr_t)qual, g0 = q0 & ~(uintptr_t)15; // the aligned group of the first quality byte
    const uint64_t n_groups = ((q0 + len - 1) >> 4) - (g0 >> 4) + 1;
    uint32_t cnt = 0;
    for (uint64_t g = part * KID_MASK_TEAM + lane; g < n_groups; g += parts * KID_MASK_TEAM) {
        const uintptr_t ga = g0 + (g << 4);
        const uint4 v = *reinterpret_cast<const uint4 *>(ga);
        uint32_t m = kid_mask_pack4(kid_mask_below(v.x, t_ones)) | kid_mask_pack4(kid_mask_below(v.y, t_ones)) << 4 |
                     kid_mask_pack4(kid_mask_below(v.z, t_ones)) << 8 | kid_mask_pack4(kid_mask_below(v.w, t_ones)) << 12;
        // bit j of m is quality byte ga + j = index i0 + j of the span; only 0 <= i0 + j < len count
        const int64_t i0 = (int64_t)(ga - q0); // -15 .. len - 1
        if (i0 < 0) m &= 0xFFFFu << (uint32_t)(-i0);
        if ((uint64_t)(i0 + 16) > len) m &= 0xFFFFu >> (uint32_t)((uint64_t)(i0 + 16) - len);
        cnt += (uint32_t)__popc(m);
        while (m) { // rare: a byte store per masked base
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            seq[i0 + (int64_t)j] = (uint8_t)'N';
            m &= m - 1u;
        }
    }
    return cnt;
}

template <bool RECS>
__global__ __launch_bounds__(KID_MASK_BLOCK) void kid_mask_kernel(uint8_t *bases, const uint8_t *quals, const KidFastqRec *recs,
                                                                    const uint64_t *offsets, uint64_t n, uint32_t threshold,
                                                                    unsigned long long *n_masked)
{
    const uint32_t lane = threadIdx.x % KID_MASK_TEAM;
    const uint64_t team = (blockIdx.x * (uint64_t)KID_MASK_BLOCK + threadIdx.x) / KID_MASK_TEAM;
    const uint64_t teams = (uint64_t)gridDim.x * (KID_MASK_BLOCK / KID_MASK_TEAM);
    const uint32_t t_ones = threshold * 0x01010101u;
    uint32_t cnt = 0;
    if (RECS) {
        for (uint64_t r = team; r < n; r += teams) {
            const KidFastqRec rc = recs[r];
            if (rc.qual_len < rc.seq_len) continue;
            cnt += kid_mask_span(bases + rc.seq_off, quals + rc.qual_off, rc.seq_len, blockIdx.y, gridDim.y, lane, t_ones);
        }
    } else {
        const uint64_t b0 = offsets[0], b1 = offsets[n];
        if (b1 > b0) cnt = kid_mask_span(bases + b0, quals + b0, b1 - b0, team, teams, lane, t_ones);
    }
    if (!n_masked) return;
    __shared__ unsigned long long s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    unsigned long long c = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (unsigned long long)__shfl_xor((long long)c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(n_masked, s_cnt);
}
