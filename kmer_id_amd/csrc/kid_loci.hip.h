// kid_loci.hip.h -- place reads on a genome by colinear hits (kid_db_read_loci*): one record per read from the hits of a
// batch and the sites of the database (org and pos per entry, kid_db_set_sites), a pure function of the MULTISET of a
// read's (pos, entry) pairs; targets play no role.
// Input: the CSR of kid_hits.hip.h and the windows looked up per read, as for kid_support.hip.h.  For one read with hits
// h_1 .. h_m, n windows and the diagonal bin W >= 1:
//   participants the first min(m, KID_LOCI_MAX_HITS) hits whose entry < n_entries
//   keys         of a participant with g = org[entry], x = pos[entry], r = its pos in the read:
//                forward (g, 0, floor((x - r) / W)), reverse (g, 1, (x + r) / W); 64-bit, floor toward minus infinity
//   c(key)       the participants that have the key
//   best key     the largest c; ties: strand 0 first, then the lowest g, then the lowest diagonal.  The chain: the
//                participants with that key
//   record       org and strand of the best key, n_chain = its c, n_org = participants with g = org, n_other = the
//                largest c over keys of another g (0: none), n_hits = m, n_kmers = n, pos_first / pos_last = the smallest
//                and largest read position in the chain, entry_first = the entry of the chain hit at pos_first (the lowest
//                if several share it).  No participant: everything but n_hits and n_kmers is 0
// A key is one 64-bit word, strand << 58 | g << 34 | diagonal (g < 2^24; the forward diagonal biased by 2^32: x - r is
// at least -(2^32 - 1), and both stay below 2^34), so the tie order is the order of the words.
//
// What a set of keys comes to is a KidLociTop: the best (c, key) and the largest c among keys of another g, with that g.
// Two of them merge (KidLociTop::merge); the merge is associative, commutative and idempotent in what the record takes
// from it (the best (c, key) is a maximum in a total order, c2 the maximum of c over the keys of another g than the best
// one's, and a maximum is all three; g2 alone may depend on the order where two orgs tie for c2, and nobody reads it
// behind the last merge), so lanes, waves and strands may be folded in any order and a key may be offered more than once.
// The top is a template over the words of its key, compared first word first: one word here, two for the placements of
// kid_fragment_loci.hip.h, which shares everything below that has no family in its name: the top, the ends of a chain
// (KidLociEnds), a count (KidLociCount), the fold of either over a workgroup (kid_loci_fold) and the stages of the second
// kernel (kid_loci_fill_sort, kid_loci_run_starts, kid_loci_run_end).
//
// Three regimes by the read's hits m, all giving the same record:
//   m <= KID_LOCI_LANE_HITS   a lane takes the read: its keys in registers, c by pairwise tests
//   m <= KID_LOCI_WAVE_HITS   the whole wave: 64 candidate hits per tile, every lane's two keys against the keys of all m
//                             hits (computed 64 at a time and handed round by readlane); the lanes' tops merged by a butterfly
//   more                      kid_loci_kernel appends the read's index to a device list and writes nothing for it;
//                             kid_loci_big_kernel, queued behind it, takes the list with one workgroup per read: the forward
//                             keys of the participants sorted in LDS (bitonic, 32 KiB), every run's length found by a binary
//                             search from its first element, then the same for the reverse keys; the threads' tops merged
//                             through LDS.  The order of the list is not deterministic; nothing read from it depends on that.
// Behind the best key every regime passes over the participants once more for n_org and the chain's ends.
// No atomics but the list's counter; nothing is written outside `out`, the list and its counter.
#pragma once
#include "kid_calls.hip.h"

#define KID_LOCI_LANE_HITS 8u    // a read with more hits than this is taken by the whole wave
#define KID_LOCI_WAVE_HITS 256u  // ... and one with more than this by a workgroup of kid_loci_big_kernel
#define KID_LOCI_MAX_HITS 4096u  // the hits of a read that take part (= include/kmer_id_amd.h)
#define KID_LOCI_NO_KEY (~0ull)  // the keys of a hit that takes no part: equal to no participant's

struct KidLocus { // = kid_locus (include/kmer_id_amd.h)
    uint32_t org, strand, n_chain, n_org, n_other, n_hits, n_kmers, pos_first, pos_last, entry_first;
};
struct KidLociSites {
    const uint32_t *org, *pos; // per entry: org < 2^24, pos < 2^31 (kid_db_set_sites checks)
    uint64_t n_entries;
    uint32_t diag_bin; // W >= 1
};
struct KidLociBig { // the reads left to kid_loci_big_kernel
    uint32_t *list;   // uint32[n_reads]
    uint32_t *n_list; // their number: zeroed in front of kid_loci_kernel
};

__device__ __forceinline__ uint32_t kid_loci_key_org(uint64_t key) { return (uint32_t)(key >> 34) & 0xFFFFFFu; }

// What a set of keys of NK words comes to (on top).  Every word of every key has its org where a key word has it.
template <int NK> struct KidLociTop {
    uint64_t k[NK];  // the best key so far (c > 0)
    uint32_t c;      // its count; 0: no key yet
    uint32_t c2, g2; // the largest count among keys of another org than the best key's, and that org (c2 > 0)

    static __device__ __forceinline__ KidLociTop empty()
    {
        KidLociTop t;
#pragma unroll
        for (int i = 0; i < NK; i++) t.k[i] = KID_LOCI_NO_KEY;
        t.c = t.c2 = t.g2 = 0u;
        return t;
    }
    __device__ __forceinline__ uint32_t org() const { return kid_loci_key_org(k[0]); }
    // whether this one's key is before o's in the tie order: word I decides, then the words behind it
    template <int I = 0> __device__ __forceinline__ bool before(const KidLociTop &o) const
    {
        if constexpr (I == NK - 1) return k[I] < o.k[I];
        else return k[I] < o.k[I] || (k[I] == o.k[I] && before<I + 1>(o));
    }
    // this := what the keys behind this and those behind b come to together
    __device__ __forceinline__ void merge(const KidLociTop &b)
    {
        const uint32_t cc[4] = {c, c2, b.c, b.c2};
        const uint32_t gg[4] = {org(), g2, b.org(), b.g2};
        if (b.c > c || (b.c == c && b.before(*this))) {
#pragma unroll
            for (int i = 0; i < NK; i++) k[i] = b.k[i];
            c = b.c;
        }
        const uint32_t g = org();
        c2 = g2 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (gg[i] != g && cc[i] > c2) { c2 = cc[i]; g2 = gg[i]; }
    }
    __device__ __forceinline__ void add(uint64_t k0, uint32_t n)
    {
        static_assert(NK == 1, "a key of one word");
        const KidLociTop b = {{k0}, n, 0u, 0u};
        merge(b);
    }
    __device__ __forceinline__ void add(uint64_t k0, uint64_t k1, uint32_t n)
    {
        static_assert(NK == 2, "a key of two words");
        const KidLociTop b = {{k0, k1}, n, 0u, 0u};
        merge(b);
    }
    // the tops of a wave's lanes -> one, the same in every lane
    __device__ __forceinline__ void wave()
    {
        for (int s = 32; s >= 1; s >>= 1) {
            KidLociTop o;
#pragma unroll
            for (int i = 0; i < NK; i++) o.k[i] = (uint64_t)__shfl_xor((unsigned long long)k[i], s);
            o.c = (uint32_t)__shfl_xor((int)c, s);
            o.c2 = (uint32_t)__shfl_xor((int)c2, s);
            o.g2 = (uint32_t)__shfl_xor((int)g2, s);
            merge(o);
        }
        // (lanes may differ in g2 where two orgs tie for c2, which nobody reads behind this: one copy for all)
#pragma unroll
        for (int i = 0; i < NK; i++) k[i] = (uint64_t)__shfl((unsigned long long)k[i], 0);
        c = (uint32_t)__builtin_amdgcn_readlane((int)c, 0);
        c2 = (uint32_t)__builtin_amdgcn_readlane((int)c2, 0);
        g2 = (uint32_t)__builtin_amdgcn_readlane((int)g2, 0);
    }
};

// The ends of a chain, and a count beside them that the family gives its meaning (kid_loci_chain_add: n_org;
// kid_floci_chain_add: the chain's length).
struct KidLociEnds {
    unsigned long long first; // min of pos << 32 | entry over the chain
    uint32_t last, n;

    static __device__ __forceinline__ KidLociEnds empty() { return KidLociEnds{~0ull, 0u, 0u}; }
    __device__ __forceinline__ void merge(const KidLociEnds &o)
    {
        first = o.first < first ? o.first : first;
        last = o.last > last ? o.last : last;
        n += o.n;
    }
    // a hit of the chain
    __device__ __forceinline__ void add(const KidHit &h) { merge(KidLociEnds{(unsigned long long)h.pos << 32 | h.entry, h.pos, 0u}); }
    __device__ __forceinline__ void wave()
    {
        for (int s = 32; s >= 1; s >>= 1)
            merge(KidLociEnds{__shfl_xor(first, s), (uint32_t)__shfl_xor((int)last, s), (uint32_t)__shfl_xor((int)n, s)});
    }
};
struct KidLociCount {
    uint32_t n;
    __device__ __forceinline__ void merge(const KidLociCount &o) { n += o.n; }
    __device__ __forceinline__ void wave()
    {
        for (int s = 32; s >= 1; s >>= 1) n += (uint32_t)__shfl_xor((int)n, s);
    }
};

// The values of a workgroup's 256 threads (a top, ends, a count) -> one, the same in every thread, through sh[4]: every
// wave puts its own there, and behind a barrier every thread gets the four merged.  Entered and left by all 256 threads; sh
// is free again behind the workgroup's next barrier.  (The two halves are for several values at one barrier.)
template <class T> __device__ __forceinline__ void kid_loci_fold_put(T &v, T *sh)
{
    v.wave();
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
}
template <class T> __device__ __forceinline__ void kid_loci_fold_get(T &v, const T *sh)
{
    v = sh[0];
    for (uint32_t w = 1; w < 4u; w++) v.merge(sh[w]);
}
template <class T> __device__ __forceinline__ void kid_loci_fold(T &v, T *sh)
{
    kid_loci_fold_put(v, sh);
    __syncthreads();
    kid_loci_fold_get(v, sh);
}

// whether a participant with the keys fk and rk has the key ck (of either strand)
__device__ __forceinline__ bool kid_loci_has_key(uint64_t ck, uint64_t fk, uint64_t rk) { return ((ck >> 58) & 1ull ? rk : fk) == ck; }

// the two keys of a hit; KID_LOCI_NO_KEY twice when its entry is none of the database's (the CSR may be the caller's)
__device__ __forceinline__ void kid_loci_keys(const KidLociSites &s, const KidHit &h, uint64_t &fk, uint64_t &rk)
{
    fk = rk = KID_LOCI_NO_KEY;
    if ((uint64_t)h.entry >= s.n_entries) return;
    const uint64_t g = s.org[h.entry] & 0xFFFFFFu, w = s.diag_bin;
    const int64_t x = (int64_t)s.pos[h.entry], r = (int64_t)h.pos;
    int64_t df = x - r;
    uint64_t dr = (uint64_t)(x + r);
    if (w != 1) {
        df = df >= 0 ? (int64_t)((uint64_t)df / w) : -(int64_t)(((uint64_t)(-df) + w - 1) / w);
        dr /= w;
    }
    fk = g << 34 | (uint64_t)(df + (1ll << 32));
    rk = 1ull << 58 | g << 34 | dr;
}

// one participant (fk != KID_LOCI_NO_KEY) into n_org and, if it has the key `best`, the ends of the chain
__device__ __forceinline__ void kid_loci_chain_add(KidLociEnds &e, uint64_t best, uint64_t fk, uint64_t rk, const KidHit &h)
{
    e.n += kid_loci_key_org(fk) == kid_loci_key_org(best) ? 1u : 0u;
    if (kid_loci_has_key(best, fk, rk)) e.add(h);
}

// top (c > 0) and the ends of its chain -> the record's first five fields and its last three
__device__ __forceinline__ void kid_loci_settle(const KidLociTop<1> &t, const KidLociEnds &e, KidLocus &res)
{
    res.org = t.org();
    res.strand = (uint32_t)(t.k[0] >> 58) & 1u;
    res.n_chain = t.c;
    res.n_org = e.n;
    res.n_other = t.c2;
    res.pos_first = (uint32_t)(e.first >> 32);
    res.pos_last = e.last;
    res.entry_first = (uint32_t)e.first;
}

// ---- one lane, one read of 1 .. KID_LOCI_LANE_HITS hits
__device__ __forceinline__ void kid_loci_lane(const KidLociSites &s, const KidHit *h, uint32_t m, KidLocus &res)
{
    uint64_t fk[KID_LOCI_LANE_HITS], rk[KID_LOCI_LANE_HITS];
#pragma unroll
    for (uint32_t i = 0; i < KID_LOCI_LANE_HITS; i++) {
        fk[i] = rk[i] = KID_LOCI_NO_KEY;
        if (i < m) kid_loci_keys(s, h[i], fk[i], rk[i]);
    }
    KidLociTop<1> top = KidLociTop<1>::empty();
#pragma unroll
    for (uint32_t i = 0; i < KID_LOCI_LANE_HITS; i++) {
        if (fk[i] == KID_LOCI_NO_KEY) continue;
        uint32_t cf = 0, cr = 0;
#pragma unroll
        for (uint32_t j = 0; j < KID_LOCI_LANE_HITS; j++) {
            cf += fk[j] == fk[i] ? 1u : 0u;
            cr += rk[j] == rk[i] ? 1u : 0u;
        }
        top.add(fk[i], cf);
        top.add(rk[i], cr);
    }
    if (top.c == 0) return;
    KidLociEnds e = KidLociEnds::empty();
#pragma unroll
    for (uint32_t i = 0; i < KID_LOCI_LANE_HITS; i++)
        if (fk[i] != KID_LOCI_NO_KEY) kid_loci_chain_add(e, top.k[0], fk[i], rk[i], h[i]);
    kid_loci_settle(top, e, res);
}

__device__ __forceinline__ uint64_t kid_loci_readlane(uint64_t v, uint32_t j)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j) << 32;
}

// ---- the whole wave, one read of at most KID_LOCI_WAVE_HITS hits (every argument wave-uniform; so is the result)
__device__ __forceinline__ void kid_loci_wave(const KidLociSites &s, const KidHit *h, uint32_t m, uint32_t lane, KidLocus &res)
{
    KidLociTop<1> top = KidLociTop<1>::empty();
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) { // a tile of 64 candidate hits, one per lane
        uint64_t fk = KID_LOCI_NO_KEY, rk = KID_LOCI_NO_KEY;
        if (lane < m - c0) kid_loci_keys(s, h[c0 + lane], fk, rk);
        uint32_t cf = 0, cr = 0;
        for (uint32_t j0 = 0; j0 < m; j0 += 64u) { // against all m hits, 64 at a time
            const uint32_t nj = m - j0 < 64u ? m - j0 : 64u;
            uint64_t fj = fk, rj = rk;
            if (j0 != c0) {
                fj = rj = KID_LOCI_NO_KEY;
                if (lane < nj) kid_loci_keys(s, h[j0 + lane], fj, rj);
            }
            for (uint32_t q = 0; q < nj; q++) {
                cf += kid_loci_readlane(fj, q) == fk ? 1u : 0u;
                cr += kid_loci_readlane(rj, q) == rk ? 1u : 0u;
            }
        }
        if (fk != KID_LOCI_NO_KEY) {
            top.add(fk, cf);
            top.add(rk, cr);
        }
    }
    top.wave();
    if (top.c == 0) return;
    KidLociEnds e = KidLociEnds::empty();
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
        if (lane < m - c0) {
            uint64_t fk, rk;
            kid_loci_keys(s, h[c0 + lane], fk, rk);
            if (fk != KID_LOCI_NO_KEY) kid_loci_chain_add(e, top.k[0], fk, rk, h[c0 + lane]);
        }
    }
    e.wave();
    kid_loci_settle(top, e, res);
}

struct KidLociMethod {
    typedef KidLocus Result;
    static constexpr uint32_t lane_hits = KID_LOCI_LANE_HITS, wave_hits = KID_LOCI_WAVE_HITS;
    const KidLociSites &sites;
    static __device__ __forceinline__ Result empty(uint32_t n_kmers, uint32_t m) { return Result{0u, 0u, 0u, 0u, 0u, m, n_kmers, 0u, 0u, 0u}; }
    template <class Unit>
    __device__ __forceinline__ void lane(const KidHit *h, const Unit &un, Result &res) const
    {
        kid_loci_lane(sites, h, un.m, res);
    }
    template <class Unit>
    __device__ __forceinline__ void wave(const KidHit *h, uint32_t m, const Unit &, int, uint32_t lane, Result &res) const
    {
        kid_loci_wave(sites, h, m, lane, res);
    }
};

__global__ __launch_bounds__(256) void kid_loci_kernel(const uint64_t *hit_offsets, const KidHit *hits, const uint32_t *n_kmers,
                                                        uint64_t n_reads, const KidLociSites sites, KidLocus *out, const KidLociBig big)
{
    kid_calls_run<false, false>(KidCsrUnits<KidLocus>{hit_offsets, hits, n_kmers, n_reads, out, big.list, big.n_list},
                                KidLociMethod{sites}, KidSupportTally());
}

// ------------------------------------------------------------------ reads of more than KID_LOCI_WAVE_HITS hits
// keys[0, n2) of LDS ascending: n2 a power of two; entered and left by all 256 threads
__device__ __forceinline__ void kid_loci_sort(uint64_t *keys, uint32_t n2)
{
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < n2 / 2u; t += 256u) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
                const uint64_t a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0u)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
}

// keys[0, n2) of LDS <- the forward (reverse: the reverse) keys of the first p <= KID_LOCI_MAX_HITS hits at h, KID_LOCI_NO_KEY
// behind them, ascending; -> n2, the first power of two that is at least p and min_sort (a power of two; 512 and more
// keep every thread busy).  Entered and left by all 256 threads.
__device__ __forceinline__ uint32_t kid_loci_fill_sort(uint64_t *keys, uint32_t min_sort, const KidLociSites &sites, const KidHit *h, uint32_t p,
                                                       bool reverse)
{
    uint32_t n2 = min_sort;
    while (n2 < p) n2 <<= 1;
    for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
        uint64_t fk = KID_LOCI_NO_KEY, rk = KID_LOCI_NO_KEY;
        if (i < p) kid_loci_keys(sites, h[i], fk, rk);
        keys[i] = reverse ? rk : fk;
    }
    __syncthreads();
    if (p > 1u) kid_loci_sort(keys, n2); // (uniform)
    return n2;
}

// whether a run of a participant's key starts at keys[i] of the ascending keys
__device__ __forceinline__ bool kid_loci_run_starts(const uint64_t *keys, uint32_t i)
{
    return keys[i] != KID_LOCI_NO_KEY && (i == 0 || keys[i - 1] != keys[i]);
}

// the end of the run of `k` that starts at keys[i] of the ascending keys[0, n): the first index behind i whose key is larger
__device__ __forceinline__ uint32_t kid_loci_run_end(const uint64_t *keys, uint32_t i, uint32_t n, uint64_t k)
{
    uint32_t lo = i + 1u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] <= k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// (the arguments of kid_loci_kernel; the list is at most n_reads long by construction, so that number is not looked at)
__global__ __launch_bounds__(256) void kid_loci_big_kernel(const uint64_t *hit_offsets, const KidHit *hits, const uint32_t *n_kmers,
                                                            uint64_t /* n_reads */, const KidLociSites sites, KidLocus *out, const KidLociBig big)
{
    __shared__ uint64_t keys[KID_LOCI_MAX_HITS];
    __shared__ KidLociTop<1> sh_top[4];
    __shared__ KidLociEnds sh_ends[4];
    const uint32_t n_list = *big.n_list;
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        const uint32_t r = big.list[e];
        const KidHit *h = hits + hit_offsets[r];
        const uint32_t m = (uint32_t)(hit_offsets[r + 1] - hit_offsets[r]);
        const uint32_t p = m < KID_LOCI_MAX_HITS ? m : KID_LOCI_MAX_HITS;
        KidLociTop<1> top = KidLociTop<1>::empty();
        for (uint32_t strand = 0; strand < 2u; strand++) {
            const uint32_t n2 = kid_loci_fill_sort(keys, 512u, sites, h, p, strand != 0u);
            for (uint32_t i = threadIdx.x; i < p; i += 256u) // the first element of a run finds its end
                if (kid_loci_run_starts(keys, i)) top.add(keys[i], kid_loci_run_end(keys, i, n2, keys[i]) - i);
            __syncthreads(); // (the keys are overwritten next)
        }
        kid_loci_fold(top, sh_top);
        KidLocus res = KidLociMethod::empty(n_kmers[r], m);
        if (top.c != 0) { // (uniform)
            KidLociEnds ends = KidLociEnds::empty();
            for (uint32_t i = threadIdx.x; i < p; i += 256u) {
                uint64_t fk, rk;
                kid_loci_keys(sites, h[i], fk, rk);
                if (fk != KID_LOCI_NO_KEY) kid_loci_chain_add(ends, top.k[0], fk, rk, h[i]);
            }
            kid_loci_fold(ends, sh_ends);
            kid_loci_settle(top, ends, res);
        }
        if (threadIdx.x == 0) out[r] = res;
        __syncthreads(); // (sh_top and sh_ends are written again for the next read)
    }
}
