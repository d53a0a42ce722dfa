// kid_support.hip.h -- call reads by k-mer support (kid_db_read_support*): one record per read from the hits of a batch.
// Input: the CSR that kid_hits.hip.h leaves on the device ({pos, target, entry} per hit, in read-position order) and the
// windows looked up per read.  For one read with hit targets t_1 .. t_m and n windows:
//   final        process_read's left fold of the targets with msca (0 without a hit): what kid_classify_* returns
//   S(c)         hits whose target is c or a descendant of c (S(1) = m)
//   c passes     S(c) >= min_hits and 1000 * S(c) >= min_permille * n   (64-bit integers)
//   confident    the first node on final, parent(final), .., 1 that passes; 0 if none does or final = 0
// msca returns the deeper node of a lineage, so final need not be an ancestor of every hit: hits [6, 8] with 6 -> 8
// fold to 8 with S(8) = 1, S(6) = 2.
//
// With d_i = depth of the deepest common node of t_i and final, the node at depth d of final's root path has
// S = #{i : d_i >= d}: one pass over the hits, counting them by d_i, settles the whole climb.  On the ancestor rows d_i is
// the common-prefix length of kid_msca_rows (its depth-8 case included) and the nine counts live in registers.  Trees
// that do not fit the rows (db.rows == nullptr) climb parent[] and recount per candidate.
//
// This file also holds the two pieces the other families over the tree call: the left fold (kid_fold_lane, kid_fold_wave:
// the fragments' per-mate folds, the segments' lane) and the climb (kid_climb, a lane or a wave over the hits: the votes, the
// segments' lane; the workgroup's is kid_vote_big_climb of kid_votes.hip.h).  kid_support_lane and kid_support_wave are fold
// plus climb written out once more, as they were: each is kept by a timing (profiles/call_kernels/ab_parent_vs_branch.txt).
//
// Work split: the loop of kid_calls_run (kid_calls.hip.h) over the reads of the CSR; a read of at most KID_SUPPORT_LANE_HITS
// hits (0 - 4 in a metagenomic sample) is a lane's, and the wave takes every other: the lanes stride over the hits to
// count, and the ordered fold jumps from change to change of the running result (kid_jump_fold of kid_tile.hip.h) -- a
// left fold in hit order either way.  Pure and without atomics: byte-identical across runs.
#pragma once
#include "kid_calls.hip.h"

#define KID_SUPPORT_LANE_HITS 8u // a read with more hits than this is taken by the whole wave

struct KidSupport { // = kid_support (include/kmer_id_amd.h)
    uint32_t final_t, confident, n_kmers, n_hits, s_final, s_confident;
};
struct KidSupportRule {
    uint32_t min_hits, min_permille;
};

__device__ __forceinline__ bool kid_support_passes(uint32_t s, uint32_t n, const KidSupportRule &rule)
{
    return s >= rule.min_hits && 1000ull * (unsigned long long)s >= (unsigned long long)rule.min_permille * (unsigned long long)n;
}

// a hit's target as the kernels use it: the CSR of kid_db_support_from_hits_device is the caller's memory, and a value
// outside (0, ntar) must not become an index (it is read as the root)
__device__ __forceinline__ uint32_t kid_support_target(const KidDevDb &db, uint32_t t)
{
    return t - 1u < (uint32_t)db.ntar - 1u ? t : 1u;
}

// depth of the deepest common node of x and y: the `c` of kid_msca_rows
__device__ __forceinline__ uint32_t kid_support_common_depth(uint32_t x, const uint4 &rx, uint32_t y, const uint4 &ry)
{
    const uint32_t dx = rx.x & 0xFFFFu, dy = ry.x & 0xFFFFu;
    const uint64_t lo = ((uint64_t)(rx.y ^ ry.y) << 32) | ((rx.x ^ ry.x) & 0xFFFF0000u);
    const uint64_t hi = ((uint64_t)(rx.w ^ ry.w) << 32) | (rx.z ^ ry.z);
    const uint32_t f = lo ? (uint32_t)(__builtin_ctzll(lo) >> 4) : hi ? 4u + (uint32_t)(__builtin_ctzll(hi) >> 4) : 8u;
    uint32_t c = f - 1; // entries 1..f-1 agree
    c = c < dx ? c : dx;
    c = c < dy ? c : dy;
    if (c == 7 && dx == 8 && dy == 8 && x == y) c = 8; // depth-8 nodes are not stored in their own row
    return c;
}

// is c the node t or one of its ancestors (any tree shape)
__device__ __forceinline__ bool kid_support_under(const KidDevDb &db, uint32_t t, uint32_t c, int32_t dc)
{
    int32_t dt = db.depth[t];
    while (dt > dc) { t = (uint32_t)db.parent[t]; dt--; }
    return t == c;
}

// ---- the climb from a node (a fold's final, a vote's call; never 0) over the m > 0 hits at h
struct KidClimb {
    uint32_t s_node;                // S(node)
    uint32_t confident, s_confident; // the first node on node's root path that passes, and its S; 0, 0: none does
};

// the climb on the rows into a kid_support record: ge[d] = hits with d_i >= d = S(node at depth d of final's root path)
__device__ __forceinline__ void kid_support_settle_rows(uint32_t f, const uint4 &fr, const uint32_t (&ge)[9], const KidSupportRule &rule,
                                                        KidSupport &res)
{
    const uint32_t df = fr.x & 0xFFFFu;
    uint32_t conf_d = 9u;
    res.final_t = f;
#pragma unroll
    for (int d = 8; d >= 0; d--) {
        if ((uint32_t)d == df) res.s_final = ge[d];
        if ((uint32_t)d <= df && conf_d == 9u && kid_support_passes(ge[d], res.n_kmers, rule)) {
            conf_d = (uint32_t)d;
            res.s_confident = ge[d];
        }
    }
    if (conf_d != 9u) res.confident = conf_d == df ? f : conf_d == 0u ? 1u : kid_row_entry(fr, conf_d);
}

// WIDTH threads share the hits: 1, a lane on its own; 64, the lanes of a wave stride over them (every argument
// wave-uniform; so is the result).  (The workgroup's form, with its sums through LDS, is kid_vote_big_climb.)
template <bool ROWS, uint32_t WIDTH>
__device__ __forceinline__ KidClimb kid_climb(const KidDevDb &db, const KidHit *h, uint32_t m, uint32_t node, const uint4 &nr, uint32_t n_kmers,
                                              const KidSupportRule &rule)
{
    const uint32_t lane = WIDTH == 1u ? 0u : threadIdx.x & 63u;
    if (ROWS) {
        uint32_t ge[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c0 = 0; c0 < m; c0 += WIDTH) {
            const bool valid = WIDTH == 1u || lane < m - c0;
            uint32_t di = 0;
            if (valid) {
                const uint32_t t = kid_support_target(db, h[(uint64_t)c0 + lane].target);
                di = kid_support_common_depth(t, db.rows[t], node, nr);
            }
#pragma unroll
            for (int d = 0; d < 9; d++)
                ge[d] += WIDTH == 1u ? (di >= (uint32_t)d ? 1u : 0u) : (uint32_t)__popcll(__ballot(valid && di >= (uint32_t)d));
        }
        KidSupport s = {0u, 0u, n_kmers, 0u, 0u, 0u};
        kid_support_settle_rows(node, nr, ge, rule, s);
        return KidClimb{s.s_final, s.confident, s.s_confident};
    }
    KidClimb r = {0u, 0u, 0u};
    for (uint32_t c = node;;) { // candidates node, parent(node), .., 1: recount under each
        const int32_t dc = db.depth[c];
        uint32_t s = 0;
        for (uint32_t c0 = 0; c0 < m; c0 += WIDTH) {
            const bool valid = WIDTH == 1u || lane < m - c0;
            const bool under = valid && kid_support_under(db, kid_support_target(db, h[(uint64_t)c0 + lane].target), c, dc);
            s += WIDTH == 1u ? (under ? 1u : 0u) : (uint32_t)__popcll(__ballot(under));
        }
        if (c == node) r.s_node = s;
        if (kid_support_passes(s, n_kmers, rule)) { r.confident = c; r.s_confident = s; break; }
        if (c == 1u) break;
        c = (uint32_t)db.parent[c];
    }
    return r;
}

// ---- the left fold of the m hits at h -> the result (0: m = 0), fr its row when ROWS
// one lane (m <= KID_SUPPORT_LANE_HITS)
template <bool ROWS>
__device__ __forceinline__ uint32_t kid_fold_lane(const KidDevDb &db, const KidHit *h, uint32_t m, uint4 &fr)
{
    uint32_t f = 0;
    fr = make_uint4(0, 0, 0, 0);
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t t = kid_support_target(db, h[i].target);
        if (ROWS) {
            const uint4 row = db.rows[t];
            if (f == 0) { f = t; fr = row; }
            else { uint4 ro; f = kid_msca_rows(t, row, f, fr, ro); fr = ro; }
        } else {
            f = f == 0 ? t : kid_msca_climb(db, t, f);
        }
    }
    return f;
}

// the whole wave (every argument wave-uniform; so is the result)
template <bool ROWS>
__device__ __forceinline__ uint32_t kid_fold_wave(const KidDevDb &db, const KidHit *h, uint32_t m, uint32_t lane, uint4 &ufr)
{
    uint32_t uf = 0; // the running result
    ufr = make_uint4(0, 0, 0, 0);
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
        const uint32_t n = m - c0 < 64u ? m - c0 : 64u;
        const uint32_t tgt = lane < n ? kid_support_target(db, h[(uint64_t)c0 + lane].target) : 0u;
        uint4 row = make_uint4(0, 0, 0, 0);
        if (ROWS && tgt) row = db.rows[tgt];
        kid_jump_fold<ROWS>(db, tgt, row, n >= 64u ? ~0ull : ((1ull << n) - 1ull), uf, ufr);
    }
    return uf;
}

// ---- a read's record: fold plus climb.  One lane, one read of at most KID_SUPPORT_LANE_HITS hits: kid_fold_lane plus
// kid_climb<ROWS, 1>, written out.  As a call of those two, the support kernel lay 0.3 to 0.5 % above the timing rule on the
// hit-dense workload, which never runs this code, whether it was on the driver or not; with this text its six bodies are
// the parent's to the byte.
template <bool ROWS>
__device__ __forceinline__ void kid_support_lane(const KidDevDb &db, const KidHit *h, uint32_t m, const KidSupportRule &rule, KidSupport &res)
{
    uint32_t f = 0;
    if (ROWS) {
        uint4 fr = make_uint4(0, 0, 0, 0);
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t t = kid_support_target(db, h[i].target);
            const uint4 row = db.rows[t];
            if (f == 0) { f = t; fr = row; }
            else { uint4 ro; f = kid_msca_rows(t, row, f, fr, ro); fr = ro; }
        }
        uint32_t ge[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t t = kid_support_target(db, h[i].target);
            const uint32_t di = kid_support_common_depth(t, db.rows[t], f, fr);
#pragma unroll
            for (int d = 0; d < 9; d++) ge[d] += di >= (uint32_t)d ? 1u : 0u;
        }
        kid_support_settle_rows(f, fr, ge, rule, res);
    } else {
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t t = kid_support_target(db, h[i].target);
            f = f == 0 ? t : kid_msca_climb(db, t, f);
        }
        res.final_t = f;
        for (uint32_t c = f;;) { // candidates final, parent(final), .., 1: recount under each
            const int32_t dc = db.depth[c];
            uint32_t s = 0;
            for (uint32_t i = 0; i < m; i++) s += kid_support_under(db, kid_support_target(db, h[i].target), c, dc) ? 1u : 0u;
            if (c == f) res.s_final = s;
            if (kid_support_passes(s, res.n_kmers, rule)) { res.confident = c; res.s_confident = s; break; }
            if (c == 1u) break;
            c = (uint32_t)db.parent[c];
        }
    }
}

// The whole wave (every argument wave-uniform; so is the result): kid_fold_wave plus kid_climb<ROWS, 64>, written out.  As
// a call of those two it lay 0.8 % above the parent on support / dense and on fragments / dense and 1.2 to 2.0 % on
// segments / megabase, outside the timing rule in both samples.  A change to either copy belongs in both.
template <bool ROWS>
__device__ __forceinline__ void kid_support_wave(const KidDevDb &db, const KidHit *h, uint32_t m, const KidSupportRule &rule, uint32_t lane,
                                                 KidSupport &res)
{
    uint32_t uf = 0; // the running result
    uint4 ufr = make_uint4(0, 0, 0, 0);
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
        const uint32_t n = m - c0 < 64u ? m - c0 : 64u;
        const uint32_t tgt = lane < n ? kid_support_target(db, h[(uint64_t)c0 + lane].target) : 0u;
        uint4 row = make_uint4(0, 0, 0, 0);
        if (ROWS && tgt) row = db.rows[tgt];
        kid_jump_fold<ROWS>(db, tgt, row, n >= 64u ? ~0ull : ((1ull << n) - 1ull), uf, ufr);
    }
    if (ROWS) {
        uint32_t ge[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
            const bool valid = lane < m - c0;
            uint32_t di = 0;
            if (valid) {
                const uint32_t t = kid_support_target(db, h[(uint64_t)c0 + lane].target);
                di = kid_support_common_depth(t, db.rows[t], uf, ufr);
            }
#pragma unroll
            for (int d = 0; d < 9; d++) ge[d] += (uint32_t)__popcll(__ballot(valid && di >= (uint32_t)d));
        }
        kid_support_settle_rows(uf, ufr, ge, rule, res);
    } else {
        res.final_t = uf;
        for (uint32_t c = uf;;) {
            const int32_t dc = db.depth[c];
            uint32_t s = 0;
            for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
                const bool valid = lane < m - c0;
                const bool under = valid && kid_support_under(db, kid_support_target(db, h[(uint64_t)c0 + lane].target), c, dc);
                s += (uint32_t)__popcll(__ballot(under));
            }
            if (c == uf) res.s_final = s;
            if (kid_support_passes(s, res.n_kmers, rule)) { res.confident = c; res.s_confident = s; break; }
            if (c == 1u) break;
            c = (uint32_t)db.parent[c];
        }
    }
}

// the method of kid_segments_kernel (the methods of kid_calls_run hold references to their kernel's arguments).  Its lane
// calls the shared fold and climb: with kid_support_lane there, segments / megabase 1000:500 lay 0.65 % above in both samples.
template <bool ROWS>
struct KidSupportMethod {
    typedef KidSupport Result;
    static constexpr uint32_t lane_hits = KID_SUPPORT_LANE_HITS, wave_hits = 0u;
    const KidDevDb &db;
    const KidSupportRule &rule;
    static __device__ __forceinline__ Result empty(uint32_t n_kmers, uint32_t m) { return Result{0u, 0u, n_kmers, m, 0u, 0u}; }
    template <class Unit>
    __device__ __forceinline__ void lane(const KidHit *h, const Unit &un, Result &res) const
    {
        uint4 fr;
        const uint32_t f = kid_fold_lane<ROWS>(db, h, un.m, fr);
        const KidClimb c = kid_climb<ROWS, 1u>(db, h, un.m, f, fr, res.n_kmers, rule);
        res.final_t = f;
        res.s_final = c.s_node;
        res.confident = c.confident;
        res.s_confident = c.s_confident;
    }
    template <class Unit>
    __device__ __forceinline__ void wave(const KidHit *h, uint32_t m, const Unit &, int, uint32_t lane, Result &res) const
    {
        kid_support_wave<ROWS>(db, h, m, rule, lane, res);
    }
};

// The loop is that of kid_calls_run (kid_calls.hip.h) over the reads of a CSR, written out as it was: on the driver the kernel
// lay 0.5 % above the timing rule on the hit-dense workload in both samples.
template <bool ROWS, bool TALLY, bool DEPTH>
__global__ __launch_bounds__(256) void kid_support_kernel(const KidDevDb db, const uint64_t *hit_offsets, const KidHit *hits,
                                                           const uint32_t *n_kmers, uint64_t n_reads, const KidSupportRule rule,
                                                           KidSupport *out /* nullable */, const KidSupportTally tally)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; r0 < n_reads; r0 += n_waves * 64u) {
        const uint64_t r = r0 + lane;
        const bool have = r < n_reads;
        uint64_t h0 = 0;
        KidSupport res = {0u, 0u, 0u, 0u, 0u, 0u};
        if (have) {
            h0 = hit_offsets[r];
            res.n_hits = (uint32_t)(hit_offsets[r + 1] - h0);
            res.n_kmers = n_kmers[r];
        }
        const uint32_t m = res.n_hits;
        bool counted = false;
        if (TALLY) counted = have && (!tally.fastq_desc || tally.fastq_desc[r].n_kmers > 0);
        if (m > 0 && m <= KID_SUPPORT_LANE_HITS) {
            kid_support_lane<ROWS>(db, hits + h0, m, rule, res);
            if (TALLY && counted && res.confident > 0)
                for (uint32_t i = 0; i < m; i++) kid_support_tally_hit<DEPTH>(tally, hits[h0 + i]);
        }
        uint64_t big = __ballot(m > KID_SUPPORT_LANE_HITS);
        while (big) { // the reads of the 64 with more hits: the whole wave, one after the other
            const int j = __builtin_ctzll(big);
            big &= big - 1ull;
            const KidHit *wh = hits + (uint64_t)__shfl((unsigned long long)h0, j);
            const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane((int)m, j);
            KidSupport w = {0u, 0u, (uint32_t)__builtin_amdgcn_readlane((int)res.n_kmers, j), wm, 0u, 0u};
            kid_support_wave<ROWS>(db, wh, wm, rule, lane, w);
            if (TALLY && w.confident > 0 && ((__ballot(counted) >> j) & 1ull))
                for (uint32_t c0 = 0; c0 < wm; c0 += 64u)
                    if (lane < wm - c0) kid_support_tally_hit<DEPTH>(tally, wh[(uint64_t)c0 + lane]);
            if (lane == (uint32_t)j) res = w;
        }
        if (have && out) out[r] = res;
        if (TALLY) {
            const uint64_t zeros = __ballot(counted && res.confident == 0); // half of a metagenomic sample: one add per wave
            if (lane == 0 && zeros) atomicAdd(&tally.gcount[0], (unsigned long long)__popcll(zeros));
            if (counted && res.confident != 0) atomicAdd(&tally.gcount[res.confident], 1ull);
        }
    }
}
