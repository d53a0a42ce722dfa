// kid_fragment_votes.hip.h -- call mate pairs by root-path votes (kid_db_read_fragment_votes*): one record per fragment
// from the hits of a batch.  Input: the interleaved CSR of kid_fragments.hip.h (read 2i = mate 1 of fragment i, read
// 2i + 1 = its mate 2).  With a_1 .. a_p the hits of mate 1, b_1 .. b_q those of mate 2 and n_1, n_2 the mates' n_kmers:
//   the multiset   {a_1 .. a_p} + {b_1 .. b_q}: the contiguous span [off[2i], off[2i + 2]) of the CSR, m = p + q hits,
//                  n = n_1 + n_2 windows (uint32, the wrap of kid_fragment.n_kmers); the mate boundary is at off[2i + 1]
//   eight fields   call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident: the kid_vote record
//                  (kid_votes.hip.h) of a read with those m hits and that n under (min_hits, min_permille)
//   call_1         the vote call of a_1 .. a_p alone, call_2 that of b_1 .. b_q alone; each 0 without a hit
// Everything is a function of the two multisets: a permutation inside a mate changes nothing, an exchange of the mates
// exchanges call_1 and call_2.
//
// Work split: that of kid_vote_kernel by the fragment's total m (the loop of kid_calls_run, over the fragments of the CSR).
//   m <= KID_VOTE_LANE_HITS   a lane; m <= KID_VOTE_WAVE_HITS the whole wave.  ONE pairwise pass feeds three best sets: the
//                             MATES form of kid_vote_lane / kid_vote_wave (kid_votes.hip.h).  A fragment with p = 0 or
//                             q = 0 is a read: its per-mate calls are 0 and call.  A lane gets that from the MATES pass
//                             itself (the other mate's set is the span's, the empty mate's stays empty); the wave takes
//                             the pass without MATES for such a fragment and copies call (kid_fragment_vote_one_mate)
//   more                      the fragment's index goes to the list; kid_fragment_vote_big_kernel, queued behind, takes
//                             it with one workgroup over its row: stages 1-3 and 5 of kid_vote_big_kernel
//                             (kid_vote_big_best, kid_vote_big_clear) once per mate span when both hold hits, then
//                             stages 1-5 over the whole span.  The row is zero between rounds, fragments and calls.
// The TALLY variants count as kid_fragment_kernel does (gcount[confident]++ once per counted fragment; a fragment is
// counted when at least one mate was kept), in whichever kernel settles the fragment.
#pragma once
#include "kid_votes.hip.h"

struct KidFragmentVote { // = kid_fragment_vote (include/kmer_id_amd.h)
    uint32_t call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident, call_1, call_2;
};

// a fragment with one mate's hits alone: its per-mate calls from the span's
__device__ __forceinline__ void kid_fragment_vote_one_mate(uint32_t p, uint32_t call, uint32_t &call_1, uint32_t &call_2)
{
    call_1 = p == 0 ? 0u : call;
    call_2 = p == 0 ? call : 0u;
}

// tally.fastq_desc: the descriptors of the 2 F reads; a fragment is counted when at least one of its mates was kept.
// big.list holds fragment indexes (uint32[n_fragments]).  The loop is that of kid_calls_run (kid_calls.hip.h) over the
// fragments of the CSR, written out: on the driver the <true, true, true> form went from 79 to 83 VGPRs and from 6 to 5
// waves per SIMD (-Rpass-analysis=kernel-resource-usage), so this kernel stays off it.
template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_fragment_vote_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                                 const uint32_t *n_kmers, uint64_t n_fragments, const KidSupportRule rule,
                                                                 KidFragmentVote *out /* nullable */, const KidSupportTally tally,
                                                                 const KidVoteBig big)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t f0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; f0 < n_fragments; f0 += n_waves * 64u) {
        const uint64_t f = f0 + lane;
        const bool have = f < n_fragments;
        uint64_t h0 = 0;
        uint32_t p = 0;
        KidFragmentVote res = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (have) {
            h0 = hit_offsets[2u * f];
            p = (uint32_t)(hit_offsets[2u * f + 1] - h0);
            res.n_hits = (uint32_t)(hit_offsets[2u * f + 2] - h0);
            res.n_kmers = n_kmers[2u * f] + n_kmers[2u * f + 1];
            p = p < res.n_hits ? p : res.n_hits; // (the device form's offsets are the caller's memory)
        }
        const uint32_t m = res.n_hits;
        const bool later = m > KID_VOTE_WAVE_HITS; // kid_fragment_vote_big_kernel's: nothing is written or counted for it here
        if (later) big.list[atomicAdd(big.n_list, 1u)] = (uint32_t)f;
        bool counted = false;
        if (TALLY)
            counted = have && !later && (!tally.fastq_desc || tally.fastq_desc[2u * f].n_kmers > 0 || tally.fastq_desc[2u * f + 1].n_kmers > 0);
        if (m > 0 && m <= KID_VOTE_LANE_HITS) { // (one path for the 64 lanes, whatever their p: a branch on it would run both)
            kid_vote_lane<ROWS, true>(db, hits + h0, m, p, rule, res);
            if (TALLY && counted && res.confident > 0)
                for (uint32_t i = 0; i < m; i++) kid_support_tally_hit<DEPTH>(tally, hits[h0 + i]);
        }
        uint64_t wide = __ballot(m > KID_VOTE_LANE_HITS && !later);
        while (wide) { // the fragments of the 64 with more hits: the whole wave, one after the other
            const int j = __builtin_ctzll(wide);
            wide &= wide - 1ull;
            const KidHit *wh = hits + (uint64_t)__shfl((unsigned long long)h0, j);
            const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane((int)m, j);
            const uint32_t wp = (uint32_t)__builtin_amdgcn_readlane((int)p, j);
            KidFragmentVote w = {0u, 0u, (uint32_t)__builtin_amdgcn_readlane((int)res.n_kmers, j), wm, 0u, 0u, 0u, 0u, 0u, 0u};
            if (wp == 0 || wp == wm) {
                kid_vote_wave<ROWS, false>(db, wh, wm, 0u, rule, lane, w);
                kid_fragment_vote_one_mate(wp, w.call, w.call_1, w.call_2);
            } else {
                kid_vote_wave<ROWS, true>(db, wh, wm, wp, rule, lane, w);
            }
            if (TALLY && w.confident > 0 && ((__ballot(counted) >> j) & 1ull))
                for (uint32_t c0 = 0; c0 < wm; c0 += 64u)
                    if (lane < wm - c0) kid_support_tally_hit<DEPTH>(tally, wh[c0 + lane]);
            if (lane == (uint32_t)j) res = w;
        }
        if (have && !later && out) out[f] = res;
        if (TALLY) {
            const uint64_t zeros = __ballot(counted && res.confident == 0);
            if (lane == 0 && zeros) atomicAdd(&tally.gcount[0], (unsigned long long)__popcll(zeros));
            if (counted && res.confident != 0) atomicAdd(&tally.gcount[res.confident], 1ull);
        }
    }
}

// ------------------------------------------------------------------ fragments of more than KID_VOTE_WAVE_HITS hits
template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_fragment_vote_big_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                                     const uint32_t *n_kmers, uint64_t n_fragments, const KidSupportRule rule,
                                                                     KidFragmentVote *out /* nullable */, const KidSupportTally tally,
                                                                     const KidVoteBig big)
{
    __shared__ uint32_t sh[4 * 9]; // as in kid_vote_big_kernel
    uint32_t *row = big.rows + (uint64_t)blockIdx.x * (uint64_t)db.ntar;
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list && e < n_fragments; e += gridDim.x) {
        const uint64_t f = big.list[e];
        const uint64_t h0 = hit_offsets[2u * f];
        const KidHit *h = hits + h0;
        const uint32_t m = (uint32_t)(hit_offsets[2u * f + 2] - h0);
        uint32_t p = (uint32_t)(hit_offsets[2u * f + 1] - h0);
        p = p < m ? p : m;
        KidVote res = {0u, 0u, n_kmers[2u * f] + n_kmers[2u * f + 1], m, 0u, 0u, 0u, 0u};
        uint32_t best, nb, call, call_1 = 0, call_2 = 0;
        uint4 cr;
        if (p > 0 && p < m) { // a round per mate: its best set alone, no climb; the row is zero again behind each
            kid_vote_big_best<ROWS>(db, row, h, p, sh, best, nb, call_1, cr);
            kid_vote_big_clear(db, row, h, p);
            kid_vote_big_best<ROWS>(db, row, h + p, m - p, sh, best, nb, call_2, cr);
            kid_vote_big_clear(db, row, h + p, m - p);
        }
        kid_vote_big_best<ROWS>(db, row, h, m, sh, best, nb, call, cr);
        res.p_best = best;
        res.n_best = nb;
        kid_vote_big_climb<ROWS>(db, h, m, sh, call, cr, rule, res);
        if (p == 0 || p == m) kid_fragment_vote_one_mate(p, res.call, call_1, call_2);
        if (threadIdx.x == 0 && out)
            out[f] = KidFragmentVote{res.call, res.confident, res.n_kmers, res.n_hits, res.p_best, res.n_best, res.s_call, res.s_confident, call_1, call_2};
        if (TALLY && (!tally.fastq_desc || tally.fastq_desc[2u * f].n_kmers > 0 || tally.fastq_desc[2u * f + 1].n_kmers > 0)) {
            if (threadIdx.x == 0) atomicAdd(&tally.gcount[res.confident], 1ull);
            if (res.confident > 0)
                for (uint32_t i = threadIdx.x; i < m; i += 256u) kid_support_tally_hit<DEPTH>(tally, h[i]);
        }
        kid_vote_big_clear(db, row, h, m);
    }
}
