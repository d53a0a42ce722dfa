// kid_fragment_loci.hip.h -- place mate pairs as one fragment by colinear hits (kid_db_read_fragment_loci*): one record per
// fragment from the hits of an interleaved batch (read 2i = mate 1 of fragment i, read 2i + 1 = its mate 2) and the sites of
// the database, a pure function of the two MULTISETS of (pos, entry) pairs; targets play no role.
// The participants of a mate and their two keys are exactly those of kid_loci.hip.h (kid_loci_keys, the same key word).
// With F_s(g, D) the participants of mate s that have the forward key (g, D), R_s(g, E) those with the reverse key (g, E),
// W the diagonal bin and max_span in bases:
//   paired placement (o, g, D, E)  o = 0: F_1(g, D) >= 1 and R_2(g, E) >= 1; o = 1: F_2 and R_1.  Allowed when D <= E and
//                                  (E - D) * W <= max_span, i.e. E - D <= reach = max_span / W.  Score: the two counts' sum
//   solo placement (s, t, g, d)    one key of one mate, t = 0 forward, 1 reverse; score: its count
//   best placement                 the highest score; a paired one before a solo one; paired ones by (o, g, D, E), solo ones
//                                  by (t, g, d, s) ascending
//   record                         include/kmer_id_amd.h (kid_fragment_locus) has every field
// A placement is two 64-bit words whose order (k1, then k2) is the tie order among equal scores:
//   paired  k1 = o << 58 | g << 34 | D + 2^32 (the forward key word with o in the strand bit), k2 = the reverse key word
//   solo    k1 = 1 << 63 | the key word, k2 = s - 1
// The forward diagonal is biased by 2^32 inside the key word and the reverse one is not: kid_floci_pair takes the bias off
// before it compares D with E.
//
// What a set of placements comes to is a KidFlociTop: the best (c, k1, k2) and the largest score among placements of another
// org, with that org.  Two of them merge (kid_floci_top_merge); the merge is associative, commutative and idempotent in
// what the record takes from it, so lanes, waves and the two orientations fold in any order, and a placement may be offered
// more than once.
//
// Two regimes by the mates' hits (m_1, m_2), both giving the same record:
//   both <= KID_FLOCI_LANE_HITS   a lane takes the fragment: the keys of both mates in registers, counts and pairs by
//                                 pairwise tests.  With a sparse probe database this is nearly every fragment.
//   else                          kid_fragment_loci_kernel appends the fragment's index to a device list and writes nothing
//                                 for it; kid_fragment_loci_big_kernel, queued behind it (the kernel boundary orders the
//                                 two: no fence, no flag), takes the list with one workgroup per fragment.  For each
//                                 orientation it sorts the forward keys of one mate and the reverse keys of the other in LDS
//                                 (two lists of KID_LOCI_MAX_HITS keys, 64 KiB), and the thread at the first element of a
//                                 forward run finds the run's length by a binary search (the solo placement), then the lower
//                                 bound of its partner range [D, D + reach] on the same org in the reverse list, and walks
//                                 the runs in that range, each run's end by one more binary search.  The first elements of
//                                 the reverse runs give the reverse solos.
// The partner walk is O(forward runs x reverse runs in range) binary searches in the worst case -- a fragment of two times
// 4096 hits on one org whose diagonals all differ and all lie within max_span: 16 M pairs.  That is the cost of the rule
// (every allowed pair is a placement), not of the method.
// Behind the best placement both regimes pass over the participants once more for n_org and the two chains' ends.
// No atomics but the list's counter; every output word has one writer; nothing is written outside `out`, the list and its
// counter.  The order of the list is not deterministic; nothing read from it depends on that.
#pragma once
#include "kid_loci.hip.h"

#define KID_FLOCI_LANE_HITS 4u // a fragment with more hits than this in either mate is left to kid_fragment_loci_big_kernel
#define KID_FLOCI_MIN_SORT 64u  // the shortest list the workgroup kernel sorts: most of its fragments have a few dozen hits
#define KID_FLOCI_SOLO (1ull << 63)
#define KID_FLOCI_DIAG_MASK ((1ull << 34) - 1ull)

struct KidFragmentLocus { // = kid_fragment_locus (include/kmer_id_amd.h)
    uint32_t org, orient, mates, n_chain, n_chain_1, n_chain_2, n_org, n_other, n_hits, n_kmers, lo, hi, pos_first_1, pos_last_1, pos_first_2,
        pos_last_2;
};
struct KidFlociRule {
    uint32_t reach; // max_span / diag_bin: the largest E - D of an allowed pair
    uint32_t k;     // the database's k-mer length
};
struct KidFlociTop {
    uint64_t k1, k2; // the best placement so far (c > 0)
    uint32_t c;      // its score; 0: no placement yet
    uint32_t c2, g2; // the largest score among placements of another org than the best one's, and that org (c2 > 0)
};
struct KidFlociEnds { // of one mate's chain
    unsigned long long first; // min of pos << 32 | entry over the chain
    uint32_t last, n;
};

__device__ __forceinline__ uint32_t kid_floci_org(uint64_t k1) { return (uint32_t)(k1 >> 34) & 0xFFFFFFu; }

__device__ __forceinline__ KidFlociTop kid_floci_top_empty()
{
    KidFlociTop t = {~0ull, ~0ull, 0u, 0u, 0u};
    return t;
}

// a := what the placements behind a and those behind b come to together
__device__ __forceinline__ void kid_floci_top_merge(KidFlociTop &a, const KidFlociTop &b)
{
    const uint32_t cc[4] = {a.c, a.c2, b.c, b.c2};
    const uint32_t gg[4] = {kid_floci_org(a.k1), a.g2, kid_floci_org(b.k1), b.g2};
    if (b.c > a.c || (b.c == a.c && (b.k1 < a.k1 || (b.k1 == a.k1 && b.k2 < a.k2)))) { a.k1 = b.k1; a.k2 = b.k2; a.c = b.c; }
    const uint32_t g = kid_floci_org(a.k1);
    a.c2 = a.g2 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (gg[i] != g && cc[i] > a.c2) { a.c2 = cc[i]; a.g2 = gg[i]; }
}

__device__ __forceinline__ void kid_floci_top_add(KidFlociTop &a, uint64_t k1, uint64_t k2, uint32_t c)
{
    const KidFlociTop b = {k1, k2, c, 0u, 0u};
    kid_floci_top_merge(a, b);
}

// the solo placement of mate s (0 or 1) on `key` (a key word of either strand) with count c
__device__ __forceinline__ void kid_floci_solo(KidFlociTop &a, uint64_t key, uint32_t c, uint32_t s)
{
    kid_floci_top_add(a, KID_FLOCI_SOLO | key, (uint64_t)s, c);
}

// the paired placement of orientation o on the forward key fk (count cf) and the reverse key rk (count cr), if it is allowed
__device__ __forceinline__ void kid_floci_pair(KidFlociTop &a, const KidFlociRule &rule, uint32_t o, uint64_t fk, uint32_t cf, uint64_t rk, uint32_t cr)
{
    if (kid_floci_org(fk) != kid_floci_org(rk)) return;
    const int64_t D = (int64_t)(fk & KID_FLOCI_DIAG_MASK) - (1ll << 32), E = (int64_t)(rk & KID_FLOCI_DIAG_MASK);
    if (D > E || E - D > (int64_t)rule.reach) return;
    kid_floci_top_add(a, fk | (uint64_t)o << 58, rk, cf + cr);
}

// the tops of a wave's lanes -> one, the same in every lane
__device__ __forceinline__ void kid_floci_top_wave(KidFlociTop &t)
{
    for (int s = 32; s >= 1; s >>= 1) {
        KidFlociTop o;
        o.k1 = (uint64_t)__shfl_xor((unsigned long long)t.k1, s);
        o.k2 = (uint64_t)__shfl_xor((unsigned long long)t.k2, s);
        o.c = (uint32_t)__shfl_xor((int)t.c, s);
        o.c2 = (uint32_t)__shfl_xor((int)t.c2, s);
        o.g2 = (uint32_t)__shfl_xor((int)t.g2, s);
        kid_floci_top_merge(t, o);
    }
    // (lanes may differ in g2 where two orgs tie for c2, which nobody reads behind this: one copy for all)
    t.k1 = (uint64_t)__shfl((unsigned long long)t.k1, 0);
    t.k2 = (uint64_t)__shfl((unsigned long long)t.k2, 0);
    t.c = (uint32_t)__builtin_amdgcn_readlane((int)t.c, 0);
    t.c2 = (uint32_t)__builtin_amdgcn_readlane((int)t.c2, 0);
    t.g2 = (uint32_t)__builtin_amdgcn_readlane((int)t.g2, 0);
}

// What the best placement chooses: the key word of each mate's chain (KID_LOCI_NO_KEY: the mate is not in the placement).
__device__ __forceinline__ void kid_floci_chosen(const KidFlociTop &t, uint64_t ck[2])
{
    ck[0] = ck[1] = KID_LOCI_NO_KEY;
    if (t.k1 & KID_FLOCI_SOLO)
        ck[t.k2 & 1ull] = t.k1 & ~KID_FLOCI_SOLO;
    else {
        const uint32_t o = (uint32_t)(t.k1 >> 58) & 1u; // the forward mate is mate 1 + o
        ck[o] = t.k1 & ~(1ull << 58);
        ck[1u - o] = t.k2;
    }
}

__device__ __forceinline__ KidFlociEnds kid_floci_ends_empty()
{
    KidFlociEnds e = {~0ull, 0u, 0u};
    return e;
}

// one participant of a mate (fk != KID_LOCI_NO_KEY) into n_org and, if it has the mate's chosen key ck, the chain's ends
__device__ __forceinline__ void kid_floci_ends_add(KidFlociEnds &e, uint32_t &n_org, uint32_t org, uint64_t ck, uint64_t fk, uint64_t rk,
                                                   const KidHit &h)
{
    n_org += kid_floci_org(fk) == org ? 1u : 0u;
    if (ck != KID_LOCI_NO_KEY && ((ck >> 58) & 1ull ? rk : fk) == ck) {
        const unsigned long long p = (unsigned long long)h.pos << 32 | h.entry;
        e.first = p < e.first ? p : e.first;
        e.last = h.pos > e.last ? h.pos : e.last;
        e.n++;
    }
}

__device__ __forceinline__ void kid_floci_ends_merge(KidFlociEnds &e, unsigned long long first, uint32_t last, uint32_t n)
{
    e.first = first < e.first ? first : e.first;
    e.last = last > e.last ? last : e.last;
    e.n += n;
}

__device__ __forceinline__ void kid_floci_ends_wave(KidFlociEnds &e)
{
    for (int s = 32; s >= 1; s >>= 1)
        kid_floci_ends_merge(e, __shfl_xor(e.first, s), (uint32_t)__shfl_xor((int)e.last, s), (uint32_t)__shfl_xor((int)e.n, s));
}

// top (c > 0), its chosen keys and the ends of the two chains -> every field of the record but n_hits and n_kmers
__device__ __forceinline__ void kid_floci_settle(const KidLociSites &s, const KidFlociRule &rule, const KidFlociTop &t, const uint64_t ck[2],
                                                 const KidFlociEnds e[2], uint32_t n_org, KidFragmentLocus &res)
{
    res.org = kid_floci_org(t.k1);
    res.mates = (ck[0] != KID_LOCI_NO_KEY ? 1u : 0u) | (ck[1] != KID_LOCI_NO_KEY ? 2u : 0u);
    // 0: mate 1 reads forward -- its own key is forward, or mate 2's is reverse
    res.orient = ck[0] != KID_LOCI_NO_KEY ? (uint32_t)(ck[0] >> 58) & 1u : 1u - ((uint32_t)(ck[1] >> 58) & 1u);
    res.n_chain = t.c;
    res.n_org = n_org;
    res.n_other = t.c2;
    int64_t lo = INT64_MAX, hi = 0;
    uint32_t n[2] = {0u, 0u}, first[2] = {0u, 0u}, last[2] = {0u, 0u};
#pragma unroll
    for (int m = 0; m < 2; m++) {
        if (ck[m] == KID_LOCI_NO_KEY) continue;
        n[m] = e[m].n;
        first[m] = (uint32_t)(e[m].first >> 32);
        last[m] = e[m].last;
        const int64_t a = (int64_t)s.pos[(uint32_t)e[m].first], d = (int64_t)(last[m] - first[m]);
        const bool reverse = (ck[m] >> 58) & 1ull;
        const int64_t l = reverse ? (a - d > 0 ? a - d : 0) : a;
        const int64_t h = reverse ? a + (int64_t)rule.k - 1 : a + d + (int64_t)rule.k - 1;
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    res.lo = (uint32_t)lo; // (a site: below 2^31)
    res.hi = hi > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)hi;
    res.n_chain_1 = n[0];
    res.n_chain_2 = n[1];
    res.pos_first_1 = first[0];
    res.pos_last_1 = last[0];
    res.pos_first_2 = first[1];
    res.pos_last_2 = last[1];
}

__device__ __forceinline__ KidFragmentLocus kid_floci_empty(uint32_t n_hits, uint32_t n_kmers)
{
    KidFragmentLocus r = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, n_hits, n_kmers, 0u, 0u, 0u, 0u, 0u, 0u};
    return r;
}

// ---- one lane, one fragment whose mates have at most KID_FLOCI_LANE_HITS hits each (h1, h2: the mates' hits)
__device__ __forceinline__ void kid_floci_lane(const KidLociSites &s, const KidFlociRule &rule, const KidHit *h1, uint32_t m1, const KidHit *h2,
                                               uint32_t m2, KidFragmentLocus &res)
{
    constexpr uint32_t L = KID_FLOCI_LANE_HITS;
    uint64_t fk[2][L], rk[2][L];
    uint32_t cf[2][L], cr[2][L];
#pragma unroll
    for (uint32_t i = 0; i < L; i++) {
        fk[0][i] = rk[0][i] = fk[1][i] = rk[1][i] = KID_LOCI_NO_KEY;
        if (i < m1) kid_loci_keys(s, h1[i], fk[0][i], rk[0][i]);
        if (i < m2) kid_loci_keys(s, h2[i], fk[1][i], rk[1][i]);
    }
    KidFlociTop top = kid_floci_top_empty();
#pragma unroll
    for (uint32_t m = 0; m < 2u; m++)
#pragma unroll
        for (uint32_t i = 0; i < L; i++) {
            cf[m][i] = cr[m][i] = 0;
#pragma unroll
            for (uint32_t j = 0; j < L; j++) {
                cf[m][i] += fk[m][j] == fk[m][i] ? 1u : 0u;
                cr[m][i] += rk[m][j] == rk[m][i] ? 1u : 0u;
            }
            if (fk[m][i] == KID_LOCI_NO_KEY) continue;
            kid_floci_solo(top, fk[m][i], cf[m][i], m);
            kid_floci_solo(top, rk[m][i], cr[m][i], m);
        }
#pragma unroll
    for (uint32_t i = 0; i < L; i++) {
        if (fk[0][i] == KID_LOCI_NO_KEY) continue;
#pragma unroll
        for (uint32_t j = 0; j < L; j++) {
            if (fk[1][j] == KID_LOCI_NO_KEY) continue;
            kid_floci_pair(top, rule, 0u, fk[0][i], cf[0][i], rk[1][j], cr[1][j]);
            kid_floci_pair(top, rule, 1u, fk[1][j], cf[1][j], rk[0][i], cr[0][i]);
        }
    }
    if (top.c == 0) return;
    uint64_t ck[2];
    kid_floci_chosen(top, ck);
    KidFlociEnds e[2] = {kid_floci_ends_empty(), kid_floci_ends_empty()};
    uint32_t n_org = 0;
    const uint32_t org = kid_floci_org(top.k1);
#pragma unroll
    for (uint32_t i = 0; i < L; i++) {
        if (fk[0][i] != KID_LOCI_NO_KEY) kid_floci_ends_add(e[0], n_org, org, ck[0], fk[0][i], rk[0][i], h1[i]);
        if (fk[1][i] != KID_LOCI_NO_KEY) kid_floci_ends_add(e[1], n_org, org, ck[1], fk[1][i], rk[1][i], h2[i]);
    }
    kid_floci_settle(s, rule, top, ck, e, n_org, res);
}

// hit_offsets: uint64[2 n_fragments + 1] of the interleaved batch; out: one record per fragment
__global__ __launch_bounds__(256) void kid_fragment_loci_kernel(const uint64_t *hit_offsets, const KidHit *hits, const uint32_t *n_kmers,
                                                                 uint64_t n_fragments, const KidLociSites sites, const KidFlociRule rule,
                                                                 KidFragmentLocus *out, const KidLociBig big)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_fragments; f += stride) {
        const uint64_t o0 = hit_offsets[2u * f], o1 = hit_offsets[2u * f + 1u], o2 = hit_offsets[2u * f + 2u];
        const uint32_t m1 = (uint32_t)(o1 - o0), m2 = (uint32_t)(o2 - o1);
        if (m1 > KID_FLOCI_LANE_HITS || m2 > KID_FLOCI_LANE_HITS) {
            big.list[atomicAdd(big.n_list, 1u)] = (uint32_t)f;
            continue;
        }
        KidFragmentLocus res = kid_floci_empty(m1 + m2, n_kmers[2u * f] + n_kmers[2u * f + 1u]);
        if (m1 + m2) kid_floci_lane(sites, rule, hits + o0, m1, hits + o1, m2, res);
        out[f] = res;
    }
}

// ------------------------------------------------------------------ fragments with a mate of more than KID_FLOCI_LANE_HITS hits
// the end of the run of `k` that starts at keys[i] of the ascending keys[0, n): the first index behind i whose key is larger
__device__ __forceinline__ uint32_t kid_floci_run_end(const uint64_t *keys, uint32_t i, uint32_t n, uint64_t k)
{
    uint32_t lo = i + 1u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] <= k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// keys[0, n2) <- the forward (reverse: the reverse) keys of the first p hits at h, KID_LOCI_NO_KEY behind them; sorted.
// Entered and left by all 256 threads; n2 a power of two.
__device__ __forceinline__ void kid_floci_fill_sort(uint64_t *keys, uint32_t n2, const KidLociSites &sites, const KidHit *h, uint32_t p,
                                                    bool reverse)
{
    for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
        uint64_t fk = KID_LOCI_NO_KEY, rk = KID_LOCI_NO_KEY;
        if (i < p) kid_loci_keys(sites, h[i], fk, rk);
        keys[i] = reverse ? rk : fk;
    }
    __syncthreads();
    if (p > 1u) kid_loci_sort(keys, n2); // (uniform)
}

// (the arguments of kid_fragment_loci_kernel; the list is at most n_fragments long by construction)
__global__ __launch_bounds__(256) void kid_fragment_loci_big_kernel(const uint64_t *hit_offsets, const KidHit *hits, const uint32_t *n_kmers,
                                                                     uint64_t /* n_fragments */, const KidLociSites sites,
                                                                     const KidFlociRule rule, KidFragmentLocus *out, const KidLociBig big)
{
    __shared__ uint64_t ka[KID_LOCI_MAX_HITS], kb[KID_LOCI_MAX_HITS]; // the forward keys of one mate, the reverse keys of the other
    __shared__ KidFlociTop sh_top[4];
    __shared__ KidFlociEnds sh_ends[4][2];
    __shared__ uint32_t sh_n_org[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        const uint64_t f = big.list[e];
        const uint64_t o0 = hit_offsets[2u * f], o1 = hit_offsets[2u * f + 1u], o2 = hit_offsets[2u * f + 2u];
        const KidHit *h[2] = {hits + o0, hits + o1};
        const uint32_t m[2] = {(uint32_t)(o1 - o0), (uint32_t)(o2 - o1)};
        uint32_t p[2], n2[2];
        for (int s = 0; s < 2; s++) {
            p[s] = m[s] < KID_LOCI_MAX_HITS ? m[s] : KID_LOCI_MAX_HITS;
            n2[s] = KID_FLOCI_MIN_SORT;
            while (n2[s] < p[s]) n2[s] <<= 1; // (at most KID_LOCI_MAX_HITS)
        }
        KidFlociTop top = kid_floci_top_empty();
        for (uint32_t o = 0; o < 2u; o++) { // mate A = o reads forward, mate B = 1 - o reverse
            const uint32_t A = o, B = 1u - o;
            kid_floci_fill_sort(ka, n2[A], sites, h[A], p[A], false);
            kid_floci_fill_sort(kb, n2[B], sites, h[B], p[B], true);
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < p[A]; i += 256u) { // the first element of a forward run
                const uint64_t k = ka[i];
                if (k == KID_LOCI_NO_KEY || (i > 0 && ka[i - 1] == k)) continue;
                const uint32_t cf = kid_floci_run_end(ka, i, n2[A], k) - i;
                kid_floci_solo(top, k, cf, A);
                // its partners: the reverse keys of the same org with E in [max(D, 0), D + reach]
                const int64_t D = (int64_t)(k & KID_FLOCI_DIAG_MASK) - (1ll << 32);
                int64_t e_hi = D + (int64_t)rule.reach;
                if (e_hi < 0) continue;
                e_hi = e_hi > (int64_t)KID_FLOCI_DIAG_MASK ? (int64_t)KID_FLOCI_DIAG_MASK : e_hi;
                const uint64_t base = 1ull << 58 | (uint64_t)kid_floci_org(k) << 34;
                const uint64_t r_lo = base | (uint64_t)(D > 0 ? D : 0), r_hi = base | (uint64_t)e_hi;
                uint32_t lo = 0, hi = n2[B];
                while (lo < hi) { // the first key that is at least r_lo
                    const uint32_t mid = (lo + hi) >> 1;
                    if (kb[mid] < r_lo) lo = mid + 1u;
                    else hi = mid;
                }
                while (lo < n2[B]) {
                    const uint64_t r = kb[lo];
                    if (r > r_hi) break; // (KID_LOCI_NO_KEY is larger than every r_hi)
                    const uint32_t next = kid_floci_run_end(kb, lo, n2[B], r);
                    kid_floci_pair(top, rule, o, k, cf, r, next - lo);
                    lo = next;
                }
            }
            for (uint32_t i = threadIdx.x; i < p[B]; i += 256u) { // the first element of a reverse run
                const uint64_t k = kb[i];
                if (k == KID_LOCI_NO_KEY || (i > 0 && kb[i - 1] == k)) continue;
                kid_floci_solo(top, k, kid_floci_run_end(kb, i, n2[B], k) - i, B);
            }
            __syncthreads(); // (the keys are overwritten next)
        }
        kid_floci_top_wave(top);
        if (lane == 0) sh_top[wave] = top;
        __syncthreads();
        top = sh_top[0];
        for (uint32_t w = 1; w < 4u; w++) kid_floci_top_merge(top, sh_top[w]);
        KidFragmentLocus res = kid_floci_empty(m[0] + m[1], n_kmers[2u * f] + n_kmers[2u * f + 1u]);
        if (top.c != 0) { // (uniform)
            uint64_t ck[2];
            kid_floci_chosen(top, ck);
            KidFlociEnds ends[2] = {kid_floci_ends_empty(), kid_floci_ends_empty()};
            uint32_t n_org = 0;
            const uint32_t org = kid_floci_org(top.k1);
            for (int s = 0; s < 2; s++)
                for (uint32_t i = threadIdx.x; i < p[s]; i += 256u) {
                    uint64_t fk, rk;
                    kid_loci_keys(sites, h[s][i], fk, rk);
                    if (fk != KID_LOCI_NO_KEY) kid_floci_ends_add(ends[s], n_org, org, ck[s], fk, rk, h[s][i]);
                }
            kid_floci_ends_wave(ends[0]);
            kid_floci_ends_wave(ends[1]);
            for (int s = 32; s >= 1; s >>= 1) n_org += (uint32_t)__shfl_xor((int)n_org, s);
            if (lane == 0) {
                sh_ends[wave][0] = ends[0];
                sh_ends[wave][1] = ends[1];
                sh_n_org[wave] = n_org;
            }
            __syncthreads();
            ends[0] = sh_ends[0][0];
            ends[1] = sh_ends[0][1];
            n_org = sh_n_org[0];
            for (uint32_t w = 1; w < 4u; w++) {
                for (int s = 0; s < 2; s++) kid_floci_ends_merge(ends[s], sh_ends[w][s].first, sh_ends[w][s].last, sh_ends[w][s].n);
                n_org += sh_n_org[w];
            }
            if (threadIdx.x == 0) kid_floci_settle(sites, rule, top, ck, ends, n_org, res);
        }
        if (threadIdx.x == 0) out[f] = res;
        __syncthreads(); // (the shared tops and ends are written again for the next fragment)
    }
}
