// kid_fragments.hip.h -- call mate pairs as one fragment (kid_db_read_fragments*): one record per fragment from the hits
// of a batch.  Input: a hit CSR of 2 F reads in interleaved order, read 2i = mate 1 of fragment i, read 2i + 1 = its
// mate 2, as kid_hits.hip.h leaves it.  With a_1 .. a_p the hits of mate 1, b_1 .. b_q those of mate 2 and n_1, n_2 the
// mates' n_kmers:
//   the sequence   a_1 .. a_p, b_1 .. b_q: mate 1 first; m = p + q hits, n = n_1 + n_2 windows.  It is the contiguous span
//                  [off[2i], off[2i + 2]) of the CSR; the mate boundary is at off[2i + 1].  No window spans the two mates.
//   six fields     final, confident, n_kmers, n_hits, s_final, s_confident: the kid_support record (kid_support.hip.h) of
//                  that sequence with that n under (min_hits, min_permille)
//   final_1        the left fold of a_1 .. a_p alone, final_2 that of b_1 .. b_q alone; each 0 without a hit
// msca is not associative, so final is not msca(final_1, final_2) in general: it is one left fold over the m hits that
// continues from final_1 into mate 2's hits.
//
// Work split: that of kid_support_kernel by the fragment's hits in total.  The
// six fields come from kid_support_lane / kid_support_wave over the whole span.  At the mate boundary the kernel takes the
// route of three folds: the span's (inside kid_support_*), mate 1's and mate 2's, the last two (kid_fold_wave) in chunks of
// 64 counted from each mate's own first hit, so the boundary never falls inside a chunk.  A fragment with p = 0 or q = 0
// has its per-mate folds from the span's (0 and final) and folds once.
// Pure and without atomics: byte-identical across runs.  The TALLY variant counts every hit of both mates (in the DEPTH
// form a k-mer present in both mates adds 2).
#pragma once
#include "kid_support.hip.h"

struct KidFragment { // = kid_fragment (include/kmer_id_amd.h)
    uint32_t final_t, confident, n_kmers, n_hits, s_final, s_confident, final_1, final_2;
};

// The loop is that of kid_calls_run (kid_calls.hip.h) over the fragments of an interleaved CSR, written out as it was: on the
// driver the kernel lay up to 0.6 % above the timing rule on the hit-dense workload in both samples
// (profiles/call_kernels/ab_parent_vs_branch.txt).  The per-mate folds are the shared kid_fold_lane / kid_fold_wave.
// tally.fastq_desc: the descriptors of the 2 F reads; a fragment is counted when at least one of its mates was kept
template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_fragment_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                            const uint32_t *n_kmers, uint64_t n_fragments, const KidSupportRule rule,
                                                            KidFragment *out /* nullable */, const KidSupportTally tally)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t f0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; f0 < n_fragments; f0 += n_waves * 64u) {
        const uint64_t f = f0 + lane;
        const bool have = f < n_fragments;
        uint64_t h0 = 0;
        uint32_t p = 0, final_1 = 0, final_2 = 0;
        KidSupport res = {0u, 0u, 0u, 0u, 0u, 0u};
        uint4 fr; // (the per-mate folds' rows: unused)
        if (have) {
            h0 = hit_offsets[2u * f];
            p = (uint32_t)(hit_offsets[2u * f + 1] - h0);
            res.n_hits = (uint32_t)(hit_offsets[2u * f + 2] - h0);
            res.n_kmers = n_kmers[2u * f] + n_kmers[2u * f + 1];
            p = p < res.n_hits ? p : res.n_hits; // (the device form's offsets are the caller's memory)
        }
        const uint32_t m = res.n_hits;
        bool counted = false;
        if (TALLY) counted = have && (!tally.fastq_desc || tally.fastq_desc[2u * f].n_kmers > 0 || tally.fastq_desc[2u * f + 1].n_kmers > 0);
        if (m > 0 && m <= KID_SUPPORT_LANE_HITS) {
            kid_support_lane<ROWS>(db, hits + h0, m, rule, res);
            if (p == 0) final_2 = res.final_t;
            else if (p == m) final_1 = res.final_t;
            else {
                final_1 = kid_fold_lane<ROWS>(db, hits + h0, p, fr);
                final_2 = kid_fold_lane<ROWS>(db, hits + h0 + p, m - p, fr);
            }
            if (TALLY && counted && res.confident > 0)
                for (uint32_t i = 0; i < m; i++) kid_support_tally_hit<DEPTH>(tally, hits[h0 + i]);
        }
        uint64_t big = __ballot(m > KID_SUPPORT_LANE_HITS);
        while (big) { // the fragments of the 64 with more hits: the whole wave, one after the other
            const int j = __builtin_ctzll(big);
            big &= big - 1ull;
            const KidHit *wh = hits + (uint64_t)__shfl((unsigned long long)h0, j);
            const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane((int)m, j);
            const uint32_t wp = (uint32_t)__builtin_amdgcn_readlane((int)p, j);
            KidSupport w = {0u, 0u, (uint32_t)__builtin_amdgcn_readlane((int)res.n_kmers, j), wm, 0u, 0u};
            kid_support_wave<ROWS>(db, wh, wm, rule, lane, w);
            uint32_t w1 = 0, w2 = 0;
            if (wp == 0) w2 = w.final_t;
            else if (wp == wm) w1 = w.final_t;
            else {
                w1 = kid_fold_wave<ROWS>(db, wh, wp, lane, fr);
                w2 = kid_fold_wave<ROWS>(db, wh + wp, wm - wp, lane, fr);
            }
            if (TALLY && w.confident > 0 && ((__ballot(counted) >> j) & 1ull))
                for (uint32_t c0 = 0; c0 < wm; c0 += 64u)
                    if (lane < wm - c0) kid_support_tally_hit<DEPTH>(tally, wh[(uint64_t)c0 + lane]);
            if (lane == (uint32_t)j) { res = w; final_1 = w1; final_2 = w2; }
        }
        if (have && out) out[f] = KidFragment{res.final_t, res.confident, res.n_kmers, res.n_hits, res.s_final, res.s_confident, final_1, final_2};
        if (TALLY) {
            const uint64_t zeros = __ballot(counted && res.confident == 0);
            if (lane == 0 && zeros) atomicAdd(&tally.gcount[0], (unsigned long long)__popcll(zeros));
            if (counted && res.confident != 0) atomicAdd(&tally.gcount[res.confident], 1ull);
        }
    }
}
