// kid_votes.hip.h -- call reads by root-path votes (kid_db_read_votes*): one record per read from the hits of a batch,
// a pure function of the MULTISET of a read's hit targets (the fold behind `final` depends on their order).
// Input: the CSR of kid_hits.hip.h and the windows looked up per read, as for kid_support.hip.h.  For one read with hit
// targets t_1 .. t_m (values outside (0, ntar) read as the root) and n windows:
//   w(c)         #{i : t_i = c}
//   P(c)         #{i : t_i is c or an ancestor of c}: the sum of w over c's root path (a hit at the root counts for all)
//   best         max_i P(t_i); L = the distinct hit targets with P = best (no two of them on one lineage: P strictly
//                grows down a lineage of hit nodes)
//   call         the lowest common ancestor of L: the deepest node on every member's root path; 0 when m = 0
//   S(c), passes those of kid_support.hip.h
//   confident    the first node on call, parent(call), .., 1 that passes; 0 if none does or call = 0
// Every hit lies under call or above it or beside it exactly as it does for a `final`: the climb is the support kernel's
// ge[d] identity with call in the place of final.
//
// Three regimes by the read's hits m, all giving the same record:
//   m <= KID_VOTE_LANE_HITS   a lane takes the read: P by pairwise tests ("t_j is t_i or an ancestor" is, on the rows,
//                             kid_support_common_depth(t_i, t_j) == depth(t_j)), a later copy of a target skipped, the
//                             best set kept as (best, |L|, running LCA) -- a larger P starts it afresh
//   m <= KID_VOTE_WAVE_HITS   the whole wave: 64 candidates per tile, every lane against all m hits (read 64 at a time
//                             and handed round by readlane); the lanes' best sets are merged by a butterfly
//   more                      pairwise costs too much: the read goes to the list of kid_calls_run (kid_calls.hip.h);
//                             kid_vote_big_kernel, queued behind kid_vote_kernel, takes the list
//                             with one workgroup per read over a row uint32[ntar] of scratch (zero between reads):
//                             1 w into the row, 2 P(t_i) from the row along t_i's root path and its maximum, 3 every
//                             distinct member of L claimed once by a marker bit, counted and LCA-reduced, 4 the ge[d]
//                             count and the climb, 5 the touched entries put back to zero.  O(m * depth) per read on
//                             the rows (the parent[] form recounts per candidate of the climb, as kid_support_wave does).
//                             The order of the list is not deterministic; nothing read from it depends on that.
// The row is read and written through agent-scope atomics alone (they bypass the CU's L1, which RMW atomics do not
// refresh).  The TALLY variants count as kid_support_kernel does, in whichever kernel settles the read.
// kid_fragment_votes.hip.h and kid_segment_votes.hip.h call their units with the same pieces: the pairwise pass
// (kid_vote_lane, kid_vote_wave) and the stages of the second kernel (kid_vote_big_best / _climb / _clear).
#pragma once
#include "kid_support.hip.h"

#define KID_VOTE_LANE_HITS 8u   // a read with more hits than this is taken by the whole wave
#define KID_VOTE_WAVE_HITS 512u // ... and one with more than this by a workgroup of kid_vote_big_kernel
#define KID_VOTE_MARK 0x80000000u // in a row entry beside w (m < 2^31): this member of L has been claimed

struct KidVote { // = kid_vote (include/kmer_id_amd.h)
    uint32_t call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident;
};
struct KidVoteBig { // the reads left to kid_vote_big_kernel and its scratch
    uint32_t *list;   // uint32[n_reads]
    uint32_t *n_list; // their number: zeroed in front of kid_vote_kernel
    uint32_t *rows;   // one row uint32[ntar] per workgroup of kid_vote_big_kernel, zero between reads
};

// a := the lowest common ancestor of a and b (0: none yet, on either side); ar, br their rows when ROWS
template <bool ROWS>
__device__ __forceinline__ void kid_vote_lca(const KidDevDb &db, uint32_t &a, uint4 &ar, uint32_t b, const uint4 &br)
{
    if (b == 0 || a == b) return;
    if (a == 0) { a = b; ar = br; return; }
    if (ROWS) {
        const uint32_t c = kid_support_common_depth(a, ar, b, br);
        if (c == (ar.x & 0xFFFFu)) return;
        if (c == (br.x & 0xFFFFu)) { a = b; ar = br; return; }
        a = c == 0 ? 1u : kid_row_entry(ar, c); // (c < both depths: at most 7)
        ar.x = (ar.x & 0xFFFF0000u) | c;        // the row of the node at depth c: as kid_msca_rows makes it
    } else {
        uint32_t x = a, y = b;
        int32_t dx = db.depth[x], dy = db.depth[y];
        while (dx > dy) { x = (uint32_t)db.parent[x]; dx--; }
        while (dy > dx) { y = (uint32_t)db.parent[y]; dy--; }
        while (x != y) { x = (uint32_t)db.parent[x]; y = (uint32_t)db.parent[y]; }
        a = x;
    }
}

// is c the node t or one of its ancestors
template <bool ROWS>
__device__ __forceinline__ bool kid_vote_under(const KidDevDb &db, uint32_t t, const uint4 &tr, uint32_t c, const uint4 &cr)
{
    if (ROWS) return kid_support_common_depth(t, tr, c, cr) == (cr.x & 0xFFFFu);
    return kid_support_under(db, t, c, db.depth[c]);
}

// a best set (best, nb members, their LCA) takes in another; (p, n = 0): nothing on that side
template <bool ROWS>
__device__ __forceinline__ void kid_vote_merge(const KidDevDb &db, uint32_t &best, uint32_t &nb, uint32_t &call, uint4 &cr, uint32_t p,
                                               uint32_t n, uint32_t t, const uint4 &r)
{
    if (n == 0 || p < best) return;
    if (nb == 0 || p > best) { best = p; nb = n; call = t; cr = r; return; }
    nb += n;
    kid_vote_lca<ROWS>(db, call, cr, t, r);
}

__device__ __forceinline__ uint4 kid_vote_readlane(const uint4 &v, int j)
{
    return make_uint4((uint32_t)__builtin_amdgcn_readlane((int)v.x, j), (uint32_t)__builtin_amdgcn_readlane((int)v.y, j),
                      (uint32_t)__builtin_amdgcn_readlane((int)v.z, j), (uint32_t)__builtin_amdgcn_readlane((int)v.w, j));
}

// the best sets of a wave's lanes -> one, the same in every lane
template <bool ROWS>
__device__ __forceinline__ void kid_vote_wave_merge(const KidDevDb &db, uint32_t &best, uint32_t &nb, uint32_t &call, uint4 &cr)
{
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, s), on = (uint32_t)__shfl_xor((int)nb, s), ot = (uint32_t)__shfl_xor((int)call, s);
        const uint4 orow = make_uint4((uint32_t)__shfl_xor((int)cr.x, s), (uint32_t)__shfl_xor((int)cr.y, s), (uint32_t)__shfl_xor((int)cr.z, s),
                                      (uint32_t)__shfl_xor((int)cr.w, s));
        kid_vote_merge<ROWS>(db, best, nb, call, cr, ob, on, ot, orow);
    }
    // (a made row differs between lanes in the entries beyond its depth, which nobody reads: one copy for all)
    best = (uint32_t)__builtin_amdgcn_readlane((int)best, 0);
    nb = (uint32_t)__builtin_amdgcn_readlane((int)nb, 0);
    call = (uint32_t)__builtin_amdgcn_readlane((int)call, 0);
    cr = kid_vote_readlane(cr, 0);
}

// call and the climb from it (kid_climb of kid_support.hip.h) -> the record's call, s_call, confident, s_confident
template <class R>
__device__ __forceinline__ void kid_vote_climbed(R &res, uint32_t call, const KidClimb &c)
{
    res.call = call;
    res.s_call = c.s_node;
    res.confident = c.confident;
    res.s_confident = c.s_confident;
}

// The pairwise pass over the m > 0 hits at h, by one lane (kid_vote_lane, m <= KID_VOTE_LANE_HITS) or by the whole wave
// (kid_vote_wave, m <= KID_VOTE_WAVE_HITS; every argument wave-uniform, so is the result) -> the fields of R that kid_vote
// names.  MATES (R = KidFragmentVote, the first p hits are mate 1's): the one pass feeds three best sets.  While candidate i
// is tested against all m hits, "t_j is t_i or an ancestor" is counted twice, over the span (ps) and over the j of i's own
// mate (pm), and two duplicate flags are kept: an earlier copy in the span, an earlier copy in the own mate.  The candidate
// then enters the span's set with the first pair and its mate's set with the second; the per-mate sets need no climb,
// call_1 and call_2 are their LCAs (an empty mate's set stays empty).
template <bool ROWS, bool MATES, class R>
__device__ __forceinline__ void kid_vote_lane(const KidDevDb &db, const KidHit *h, uint32_t m, uint32_t p, const KidSupportRule &rule, R &res)
{
    const uint4 none = make_uint4(0, 0, 0, 0);
    uint32_t best = 0, nb = 0, call = 0, best1 = 0, nb1 = 0, call1 = 0, best2 = 0, nb2 = 0, call2 = 0;
    uint4 cr = none, cr1 = make_uint4(0, 0, 0, 0), cr2 = make_uint4(0, 0, 0, 0); // (copies of `none` that go unused without MATES keep cr in memory)
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t ti = kid_support_target(db, h[i].target);
        const uint4 ri = ROWS ? db.rows[ti] : none;
        const bool first = i < p; // candidate i is of mate 1: its own mate is [0, p), else [p, m)
        uint32_t ps = 0, pm = 0;
        bool dup = false, dupm = false;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t tj = kid_support_target(db, h[j].target);
            const bool same = tj == ti && j < i; // a later copy of a target is skipped
            const uint32_t under = kid_vote_under<ROWS>(db, ti, ri, tj, ROWS ? db.rows[tj] : none) ? 1u : 0u;
            dup = dup || same;
            ps += under;
            if constexpr (MATES) {
                const bool own = (j < p) == first;
                dupm = dupm || (same && own);
                pm += own ? under : 0u;
            }
        }
        kid_vote_merge<ROWS>(db, best, nb, call, cr, ps, dup ? 0u : 1u, ti, ri);
        if constexpr (MATES) {
            kid_vote_merge<ROWS>(db, best1, nb1, call1, cr1, pm, first && !dupm ? 1u : 0u, ti, ri);
            kid_vote_merge<ROWS>(db, best2, nb2, call2, cr2, pm, !first && !dupm ? 1u : 0u, ti, ri);
        }
    }
    res.p_best = best;
    res.n_best = nb;
    kid_vote_climbed(res, call, kid_climb<ROWS, 1u>(db, h, m, call, cr, res.n_kmers, rule));
    if constexpr (MATES) { res.call_1 = call1; res.call_2 = call2; }
}

template <bool ROWS, bool MATES, class R>
__device__ __forceinline__ void kid_vote_wave(const KidDevDb &db, const KidHit *h, uint32_t m, uint32_t p, const KidSupportRule &rule,
                                              uint32_t lane, R &res)
{
    const uint4 none = make_uint4(0, 0, 0, 0);
    uint32_t best = 0, nb = 0, call = 0, best1 = 0, nb1 = 0, call1 = 0, best2 = 0, nb2 = 0, call2 = 0;
    uint4 cr = none, cr1 = make_uint4(0, 0, 0, 0), cr2 = make_uint4(0, 0, 0, 0); // (copies of `none` that go unused without MATES keep cr in memory)
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) { // a tile of 64 candidates, one per lane
        const bool valid = lane < m - c0;
        const uint32_t i = c0 + lane;
        const uint32_t ti = valid ? kid_support_target(db, h[i].target) : 1u;
        const uint4 ri = ROWS ? db.rows[ti] : none;
        const bool first = i < p;
        uint32_t ps = 0, pm = 0;
        bool dup = false, dupm = false;
        for (uint32_t j0 = 0; j0 < m; j0 += 64u) { // against all m hits, 64 at a time, handed round by readlane
            const uint32_t nj = m - j0 < 64u ? m - j0 : 64u;
            const uint32_t tj = lane < nj ? kid_support_target(db, h[j0 + lane].target) : 1u;
            const uint4 rj = ROWS ? db.rows[tj] : none;
            for (uint32_t q = 0; q < nj; q++) {
                const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tj, (int)q);
                const uint4 r = ROWS ? kid_vote_readlane(rj, (int)q) : none;
                if (valid) {
                    const uint32_t j = j0 + q;
                    const bool same = t == ti && j < i;
                    const uint32_t under = kid_vote_under<ROWS>(db, ti, ri, t, r) ? 1u : 0u;
                    dup = dup || same;
                    ps += under;
                    if constexpr (MATES) {
                        const bool own = (j < p) == first;
                        dupm = dupm || (same && own);
                        pm += own ? under : 0u;
                    }
                }
            }
        }
        kid_vote_merge<ROWS>(db, best, nb, call, cr, ps, valid && !dup ? 1u : 0u, ti, ri);
        if constexpr (MATES) {
            kid_vote_merge<ROWS>(db, best1, nb1, call1, cr1, pm, valid && first && !dupm ? 1u : 0u, ti, ri);
            kid_vote_merge<ROWS>(db, best2, nb2, call2, cr2, pm, valid && !first && !dupm ? 1u : 0u, ti, ri);
        }
    }
    kid_vote_wave_merge<ROWS>(db, best, nb, call, cr); // (associative and commutative -- max, +, LCA: any order, one record)
    res.p_best = best;
    res.n_best = nb;
    kid_vote_climbed(res, call, kid_climb<ROWS, 64u>(db, h, m, call, cr, res.n_kmers, rule));
    if constexpr (MATES) {
        kid_vote_wave_merge<ROWS>(db, best1, nb1, call1, cr1);
        kid_vote_wave_merge<ROWS>(db, best2, nb2, call2, cr2);
        res.call_1 = call1;
        res.call_2 = call2;
    }
}

template <bool ROWS>
struct KidVoteMethod {
    typedef KidVote Result;
    static constexpr uint32_t lane_hits = KID_VOTE_LANE_HITS, wave_hits = KID_VOTE_WAVE_HITS;
    const KidDevDb &db;
    const KidSupportRule &rule;
    static __device__ __forceinline__ Result empty(uint32_t n_kmers, uint32_t m) { return Result{0u, 0u, n_kmers, m, 0u, 0u, 0u, 0u}; }
    template <class Unit>
    __device__ __forceinline__ void lane(const KidHit *h, const Unit &un, Result &res) const
    {
        kid_vote_lane<ROWS, false>(db, h, un.m, 0u, rule, res);
    }
    template <class Unit>
    __device__ __forceinline__ void wave(const KidHit *h, uint32_t m, const Unit &, int, uint32_t lane, Result &res) const
    {
        kid_vote_wave<ROWS, false>(db, h, m, 0u, rule, lane, res);
    }
};

template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_vote_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                        const uint32_t *n_kmers, uint64_t n_reads, const KidSupportRule rule,
                                                        KidVote *out /* nullable */, const KidSupportTally tally, const KidVoteBig big)
{
    kid_calls_run<TALLY, DEPTH>(KidCsrUnits<KidVote>{hit_offsets, hits, n_kmers, n_reads, out, big.list, big.n_list},
                                KidVoteMethod<ROWS>{db, rule}, tally);
}

// ------------------------------------------------------------------ reads of more than KID_VOTE_WAVE_HITS hits
__device__ __forceinline__ uint32_t kid_vote_row_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what the workgroup's threads did to the row has been done when the barrier opens
__device__ __forceinline__ void kid_vote_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
}

// P(t): the sum of w over t's root path
template <bool ROWS>
__device__ __forceinline__ uint32_t kid_vote_path_sum(const KidDevDb &db, const uint32_t *row, uint32_t t)
{
    uint32_t p = 0;
    if (ROWS) {
        const uint4 r = db.rows[t];
        const uint32_t d = r.x & 0xFFFFu;
        p = kid_vote_row_load(row + 1) & ~KID_VOTE_MARK;
#pragma unroll
        for (uint32_t e = 1; e < 8; e++)
            if (e <= d) p += kid_vote_row_load(row + kid_row_entry(r, e)) & ~KID_VOTE_MARK;
        if (d == 8u) p += kid_vote_row_load(row + t) & ~KID_VOTE_MARK; // depth-8 nodes are not stored in their own row
    } else {
        for (uint32_t c = t;; c = (uint32_t)db.parent[c]) {
            p += kid_vote_row_load(row + c) & ~KID_VOTE_MARK;
            if (c == 1u) break;
        }
    }
    return p;
}

// one value per wave through LDS -> the four, to every thread (sh: 4 words per value, free when this is entered)
__device__ __forceinline__ void kid_vote_block_share(uint32_t *sh, uint32_t v)
{
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
}

// ---- the stages of kid_vote_big_kernel, each entered by all 256 threads of a workgroup with uniform arguments
// (sh: uint32[36] of LDS, free on entry and on return; row: the workgroup's, zero on entry to stage 1)
// 1 w into the row, 2 the maximum of P over the hits, 3 L claimed, counted and LCA-reduced -> (best, nb, call, cr)
template <bool ROWS>
__device__ __forceinline__ void kid_vote_big_best(const KidDevDb &db, uint32_t *row, const KidHit *h, uint32_t m, uint32_t *sh, uint32_t &best,
                                                  uint32_t &nb, uint32_t &call, uint4 &cr)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint4 none = make_uint4(0, 0, 0, 0);
    // 1: w
    for (uint32_t i = threadIdx.x; i < m; i += 256u) atomicAdd(row + kid_support_target(db, h[i].target), 1u);
    kid_vote_sync();
    // 2: best
    best = 0;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) {
        const uint32_t p = kid_vote_path_sum<ROWS>(db, row, kid_support_target(db, h[i].target));
        best = p > best ? p : best;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, s);
        best = o > best ? o : best;
    }
    kid_vote_block_share(sh, best);
    __syncthreads();
    best = sh[0];
    for (int w = 1; w < 4; w++) best = sh[w] > best ? sh[w] : best;
    __syncthreads();
    // 3: L, each distinct member claimed by the thread that sets its marker
    uint32_t pb = 0;
    nb = call = 0;
    cr = none;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) {
        const uint32_t t = kid_support_target(db, h[i].target);
        if (kid_vote_path_sum<ROWS>(db, row, t) == best && !(atomicOr(row + t, KID_VOTE_MARK) & KID_VOTE_MARK))
            kid_vote_merge<ROWS>(db, pb, nb, call, cr, best, 1u, t, ROWS ? db.rows[t] : none);
    }
    kid_vote_wave_merge<ROWS>(db, pb, nb, call, cr);
    if (lane == 0) {
        uint32_t *s6 = sh + wave * 6u;
        s6[0] = nb; s6[1] = call; s6[2] = cr.x; s6[3] = cr.y; s6[4] = cr.z; s6[5] = cr.w;
    }
    __syncthreads();
    pb = nb = call = 0;
    cr = none;
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t *s6 = sh + w * 6u;
        kid_vote_merge<ROWS>(db, pb, nb, call, cr, best, s6[0], s6[1], make_uint4(s6[2], s6[3], s6[4], s6[5]));
    }
    __syncthreads();
}

// call and the ge[d] counts against it -> the record's last fields (the rows' climb: kid_support_settle_rows, which fills
// the support field names; with a KidClimb returned from it instead, and this function gone, kid_vote_big_kernel<true, true,
// true> and kid_segment_votes_kernel<true> went from 8 to 7 waves per SIMD: profiles/call_kernels/resource_usage.txt)
__device__ __forceinline__ void kid_vote_settle_rows(uint32_t call, const uint4 &cr, const uint32_t (&ge)[9], const KidSupportRule &rule,
                                                     KidVote &res)
{
    KidSupport s = {0u, 0u, res.n_kmers, res.n_hits, 0u, 0u};
    kid_support_settle_rows(call, cr, ge, rule, s);
    res.call = call;
    res.s_call = s.s_final;
    res.confident = s.confident;
    res.s_confident = s.s_confident;
}

// 4: S along call's root path, and the climb
template <bool ROWS>
__device__ __forceinline__ void kid_vote_big_climb(const KidDevDb &db, const KidHit *h, uint32_t m, uint32_t *sh, uint32_t call, const uint4 &cr,
                                                   const KidSupportRule &rule, KidVote &res)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (ROWS) {
        uint32_t ge[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c0 = wave * 64u; c0 < m; c0 += 256u) {
            const bool valid = lane < m - c0;
            uint32_t di = 0;
            if (valid) {
                const uint32_t t = kid_support_target(db, h[c0 + lane].target);
                di = kid_support_common_depth(t, db.rows[t], call, cr);
            }
#pragma unroll
            for (int d = 0; d < 9; d++) ge[d] += (uint32_t)__popcll(__ballot(valid && di >= (uint32_t)d));
        }
        if (lane == 0)
#pragma unroll
            for (int d = 0; d < 9; d++) sh[wave * 9u + (uint32_t)d] = ge[d];
        __syncthreads();
#pragma unroll
        for (int d = 0; d < 9; d++) ge[d] = sh[d] + sh[9 + d] + sh[18 + d] + sh[27 + d];
        __syncthreads();
        kid_vote_settle_rows(call, cr, ge, rule, res);
    } else {
        res.call = call;
        for (uint32_t c = call;;) {
            const int32_t dc = db.depth[c];
            uint32_t s = 0;
            for (uint32_t c0 = wave * 64u; c0 < m; c0 += 256u) {
                const bool valid = lane < m - c0;
                const bool under = valid && kid_support_under(db, kid_support_target(db, h[c0 + lane].target), c, dc);
                s += (uint32_t)__popcll(__ballot(under));
            }
            kid_vote_block_share(sh, s);
            __syncthreads();
            s = sh[0] + sh[1] + sh[2] + sh[3];
            __syncthreads();
            if (c == call) res.s_call = s;
            if (kid_support_passes(s, res.n_kmers, rule)) { res.confident = c; res.s_confident = s; break; }
            if (c == 1u) break;
            c = (uint32_t)db.parent[c];
        }
    }
}

// 5: the row back to zero for the workgroup's next read (and the next call's)
__device__ __forceinline__ void kid_vote_big_clear(const KidDevDb &db, uint32_t *row, const KidHit *h, uint32_t m)
{
    for (uint32_t i = threadIdx.x; i < m; i += 256u)
        __hip_atomic_store(row + kid_support_target(db, h[i].target), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    kid_vote_sync();
}

template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_vote_big_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                            const uint32_t *n_kmers, uint64_t n_reads, const KidSupportRule rule,
                                                            KidVote *out /* nullable */, const KidSupportTally tally, const KidVoteBig big)
{
    __shared__ uint32_t sh[4 * 9]; // per wave: a maximum; (nb, call, its row); the nine ge[d]; a count
    uint32_t *row = big.rows + (uint64_t)blockIdx.x * (uint64_t)db.ntar;
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list && e < n_reads; e += gridDim.x) {
        const uint32_t r = big.list[e];
        const KidHit *h = hits + hit_offsets[r];
        const uint32_t m = (uint32_t)(hit_offsets[r + 1] - hit_offsets[r]);
        KidVote res = {0u, 0u, n_kmers[r], m, 0u, 0u, 0u, 0u};
        uint32_t best, nb, call;
        uint4 cr;
        kid_vote_big_best<ROWS>(db, row, h, m, sh, best, nb, call, cr);
        res.p_best = best;
        res.n_best = nb;
        kid_vote_big_climb<ROWS>(db, h, m, sh, call, cr, rule, res);
        if (threadIdx.x == 0 && out) out[r] = res;
        if (TALLY && (!tally.fastq_desc || tally.fastq_desc[r].n_kmers > 0)) {
            if (threadIdx.x == 0) atomicAdd(&tally.gcount[res.confident], 1ull);
            if (res.confident > 0)
                for (uint32_t i = threadIdx.x; i < m; i += 256u) kid_support_tally_hit<DEPTH>(tally, h[i]);
        }
        kid_vote_big_clear(db, row, h, m);
    }
}
