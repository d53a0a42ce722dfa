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
// What a set of placements comes to is a KidFlociTop, the KidLociTop of kid_loci.hip.h over keys of two words: the best
// (c, k1, k2) and the largest score among placements of another org, with that org (k1 has the org where a key word has
// it).  The algebra of its merge is stated there: lanes, waves and the two orientations fold in any order, and a placement
// may be offered more than once.  The ends of a mate's chain, the fold over the workgroup and the stages of the second
// kernel are that file's too.
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
typedef KidLociTop<2> KidFlociTop; // k[0] = k1, k[1] = k2 of the best placement; c its score

// the solo placement of mate s (0 or 1) on `key` (a key word of either strand) with count c
__device__ __forceinline__ void kid_floci_solo(KidFlociTop &a, uint64_t key, uint32_t c, uint32_t s)
{
    a.add(KID_FLOCI_SOLO | key, (uint64_t)s, c);
}

// the paired placement of orientation o on the forward key fk (count cf) and the reverse key rk (count cr), if it is allowed
__device__ __forceinline__ void kid_floci_pair(KidFlociTop &a, const KidFlociRule &rule, uint32_t o, uint64_t fk, uint32_t cf, uint64_t rk, uint32_t cr)
{
    if (kid_loci_key_org(fk) != kid_loci_key_org(rk)) return;
    const int64_t D = (int64_t)(fk & KID_FLOCI_DIAG_MASK) - (1ll << 32), E = (int64_t)(rk & KID_FLOCI_DIAG_MASK);
    if (D > E || E - D > (int64_t)rule.reach) return;
    a.add(fk | (uint64_t)o << 58, rk, cf + cr);
}

// What the best placement chooses: the key word of each mate's chain (KID_LOCI_NO_KEY: the mate is not in the placement).
__device__ __forceinline__ void kid_floci_chosen(const KidFlociTop &t, uint64_t ck[2])
{
    ck[0] = ck[1] = KID_LOCI_NO_KEY;
    if (t.k[0] & KID_FLOCI_SOLO)
        ck[t.k[1] & 1ull] = t.k[0] & ~KID_FLOCI_SOLO;
    else {
        const uint32_t o = (uint32_t)(t.k[0] >> 58) & 1u; // the forward mate is mate 1 + o
        ck[o] = t.k[0] & ~(1ull << 58);
        ck[1u - o] = t.k[1];
    }
}

// one participant of a mate (fk != KID_LOCI_NO_KEY) into n_org and, if it has the mate's chosen key ck, the chain's ends and length
__device__ __forceinline__ void kid_floci_chain_add(KidLociEnds &e, uint32_t &n_org, uint32_t org, uint64_t ck, uint64_t fk, uint64_t rk,
                                                    const KidHit &h)
{
    n_org += kid_loci_key_org(fk) == org ? 1u : 0u;
    if (ck != KID_LOCI_NO_KEY && kid_loci_has_key(ck, fk, rk)) {
        e.add(h);
        e.n++;
    }
}

// top (c > 0), its chosen keys and the ends of the two chains -> every field of the record but n_hits and n_kmers
__device__ __forceinline__ void kid_floci_settle(const KidLociSites &s, const KidFlociRule &rule, const KidFlociTop &t, const uint64_t ck[2],
                                                 const KidLociEnds e[2], uint32_t n_org, KidFragmentLocus &res)
{
    res.org = t.org();
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
    KidFlociTop top = KidFlociTop::empty();
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
    KidLociEnds e[2] = {KidLociEnds::empty(), KidLociEnds::empty()};
    uint32_t n_org = 0;
    const uint32_t org = top.org();
#pragma unroll
    for (uint32_t i = 0; i < L; i++) {
        if (fk[0][i] != KID_LOCI_NO_KEY) kid_floci_chain_add(e[0], n_org, org, ck[0], fk[0][i], rk[0][i], h1[i]);
        if (fk[1][i] != KID_LOCI_NO_KEY) kid_floci_chain_add(e[1], n_org, org, ck[1], fk[1][i], rk[1][i], h2[i]);
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
// (the arguments of kid_fragment_loci_kernel; the list is at most n_fragments long by construction)
__global__ __launch_bounds__(256) void kid_fragment_loci_big_kernel(const uint64_t *hit_offsets, const KidHit *hits, const uint32_t *n_kmers,
                                                                     uint64_t /* n_fragments */, const KidLociSites sites,
                                                                     const KidFlociRule rule, KidFragmentLocus *out, const KidLociBig big)
{
    __shared__ uint64_t ka[KID_LOCI_MAX_HITS], kb[KID_LOCI_MAX_HITS]; // the forward keys of one mate, the reverse keys of the other
    __shared__ KidFlociTop sh_top[4];
    __shared__ KidLociEnds sh_ends[2][4];
    __shared__ KidLociCount sh_n_org[4];
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        const uint64_t f = big.list[e];
        const uint64_t o0 = hit_offsets[2u * f], o1 = hit_offsets[2u * f + 1u], o2 = hit_offsets[2u * f + 2u];
        const KidHit *h[2] = {hits + o0, hits + o1};
        const uint32_t m[2] = {(uint32_t)(o1 - o0), (uint32_t)(o2 - o1)};
        const uint32_t p[2] = {m[0] < KID_LOCI_MAX_HITS ? m[0] : KID_LOCI_MAX_HITS, m[1] < KID_LOCI_MAX_HITS ? m[1] : KID_LOCI_MAX_HITS};
        KidFlociTop top = KidFlociTop::empty();
        for (uint32_t o = 0; o < 2u; o++) { // mate A = o reads forward, mate B = 1 - o reverse
            const uint32_t A = o, B = 1u - o;
            const uint32_t na = kid_loci_fill_sort(ka, KID_FLOCI_MIN_SORT, sites, h[A], p[A], false);
            const uint32_t nb = kid_loci_fill_sort(kb, KID_FLOCI_MIN_SORT, sites, h[B], p[B], true);
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < p[A]; i += 256u) { // the first element of a forward run
                if (!kid_loci_run_starts(ka, i)) continue;
                const uint64_t k = ka[i];
                const uint32_t cf = kid_loci_run_end(ka, i, na, k) - i;
                kid_floci_solo(top, k, cf, A);
                // its partners: the reverse keys of the same org with E in [max(D, 0), D + reach]
                const int64_t D = (int64_t)(k & KID_FLOCI_DIAG_MASK) - (1ll << 32);
                int64_t e_hi = D + (int64_t)rule.reach;
                if (e_hi < 0) continue;
                e_hi = e_hi > (int64_t)KID_FLOCI_DIAG_MASK ? (int64_t)KID_FLOCI_DIAG_MASK : e_hi;
                const uint64_t base = 1ull << 58 | (uint64_t)kid_loci_key_org(k) << 34;
                const uint64_t r_lo = base | (uint64_t)(D > 0 ? D : 0), r_hi = base | (uint64_t)e_hi;
                uint32_t lo = 0, hi = nb;
                while (lo < hi) { // the first key that is at least r_lo
                    const uint32_t mid = (lo + hi) >> 1;
                    if (kb[mid] < r_lo) lo = mid + 1u;
                    else hi = mid;
                }
                while (lo < nb) {
                    const uint64_t r = kb[lo];
                    if (r > r_hi) break; // (KID_LOCI_NO_KEY is larger than every r_hi)
                    const uint32_t next = kid_loci_run_end(kb, lo, nb, r);
                    kid_floci_pair(top, rule, o, k, cf, r, next - lo);
                    lo = next;
                }
            }
            for (uint32_t i = threadIdx.x; i < p[B]; i += 256u) // the first element of a reverse run
                if (kid_loci_run_starts(kb, i)) kid_floci_solo(top, kb[i], kid_loci_run_end(kb, i, nb, kb[i]) - i, B);
            __syncthreads(); // (the keys are overwritten next)
        }
        kid_loci_fold(top, sh_top);
        KidFragmentLocus res = kid_floci_empty(m[0] + m[1], n_kmers[2u * f] + n_kmers[2u * f + 1u]);
        if (top.c != 0) { // (uniform)
            uint64_t ck[2];
            kid_floci_chosen(top, ck);
            KidLociEnds ends[2] = {KidLociEnds::empty(), KidLociEnds::empty()};
            KidLociCount n_org = {0u};
            const uint32_t org = top.org();
            for (int s = 0; s < 2; s++)
                for (uint32_t i = threadIdx.x; i < p[s]; i += 256u) {
                    uint64_t fk, rk;
                    kid_loci_keys(sites, h[s][i], fk, rk);
                    if (fk != KID_LOCI_NO_KEY) kid_floci_chain_add(ends[s], n_org.n, org, ck[s], fk, rk, h[s][i]);
                }
            kid_loci_fold_put(ends[0], sh_ends[0]); // (the three at one barrier: a fold each costs vector registers)
            kid_loci_fold_put(ends[1], sh_ends[1]);
            kid_loci_fold_put(n_org, sh_n_org);
            __syncthreads();
            kid_loci_fold_get(ends[0], sh_ends[0]);
            kid_loci_fold_get(ends[1], sh_ends[1]);
            kid_loci_fold_get(n_org, sh_n_org);
            if (threadIdx.x == 0) kid_floci_settle(sites, rule, top, ck, ends, n_org.n, res);
        }
        if (threadIdx.x == 0) out[f] = res;
        __syncthreads(); // (the shared tops, ends and counts are written again for the next fragment)
    }
}
