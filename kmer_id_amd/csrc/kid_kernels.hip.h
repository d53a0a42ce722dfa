// kid_kernels.hip.h -- gfx950 (MI355X, CDNA4) kernels of the k-mer read classifier: kid_classify_kernel, and through
// the headers it includes everything else a classify launch of the benchmark's workload executes --
//   kid_table.hip.h    device structs, cell loads, lookup in both geometries, DPP row scans, msca, ancestor rows between lanes
//   kid_prepare.hip.h  base packing; read descriptors from [start, stop] or FASTQ quality lines; the launch's argument block
//   kid_seenlog.hip.h  hit log -> seen-bitmap, bitmap -> ucount, or
//   kid_probes.hip.h   one lookup / hash / msca per thread (parity tests)
//   kid_insert.hip.h   keys and targets -> table cells
// DESIGN.md section 4 has a map of the classify kernel: which lambda exists for which instantiation, which loop calls what.
//
// All work here is integer / indexing work bounded by random reads of the hash
// table in HBM; there is no MFMA-shaped computation on this path.
//
// Data layout in HBM
//   bases   the caller's ASCII read text; the classify kernels read it as it is and pack in registers
//   table   uint4[2^log2_slots]   {key lo, key hi, target (0 = empty), insertion ordinal+1}
//                                 one 16-byte cell = one global_load_dwordx4 per probe
//   rows    uint4[ntar]           8 x u16 per taxonomy node: e0 = depth, e[d] = ancestor of
//                                 the node at depth d (d = 1..7, the node itself at d = depth)
//   parent  int32[ntar], depth int32[ntar]   (fallback for trees deeper than 8 levels)
//   seen    u32[n_entries / 32]     one bit per DB entry (insertion ordinal), per sample (-> ucount)
//   ord_target u32[n_entries]       target of entry o (what the builder was handed)
//   gcount  u64[ntar], stats u64[8] per sample
#pragma once
#include "kid_table.hip.h"
#include "kid_prepare.hip.h"
#include "kid_seenlog.hip.h"

#define KID_SEG_KMERS 960  // k-mers per read segment: 960 + 30 bases + 15 alignment slack <= 64 chunks of 16 B
#define KID_CQ_CAP 192   // the queue of unresolved lookups: a read appends at most 128 entries to fewer than KID_CQ_FLUSH queued ones
#define KID_CQ_FLUSH 64
// The LDS area of one wave, as word offsets from its start.  Three kinds of area: KidWaveLds<true, 1 or 2> of the pair
// and duo loops (no strip: their words travel by ds_bpermute; one area and one dispatch limit for both, the duo loop
// leaves the read numbers unused), <true, 0> of the general loops on the minimizer-localised table and <false, 0> of
// those on the reference table (no queue: a hit is followed up on the spot).  The members behind `total` of a kind are
// not part of it.  kid_launch_classify sizes the launch and sets its dispatch limits by `total`: 820, 792 and 104 words.
template <bool MINLOC, int PAIRK>
struct KidWaveLds {
    static constexpr uint32_t strip = 0;                           // 64 packed-base words of the staged segment + 2 of zeros
    static constexpr uint32_t mask = strip + (PAIRK ? 0 : 66);     // its invalid-base bits, 16 per word: 32 words + 2 of zeros
    static constexpr uint32_t counters = mask + (PAIRK ? 0 : 34);  // [0..1] lookups (64 bits), [2] hits, [3] probes beyond the first of a lookup
    // the queue of unresolved lookups, three columns of KID_CQ_CAP words -- key lo, key hi (or {target, ordinal} of a
    // verified hit), table line -- and one tag byte per entry: read number mod 64 (+ 0x80: verified)
    static constexpr uint32_t cq_klo = counters + 4, cq_khi = cq_klo + KID_CQ_CAP, cq_lw = cq_khi + KID_CQ_CAP;
    static constexpr uint32_t cq_tag = cq_lw + KID_CQ_CAP;
    static constexpr uint32_t results = cq_tag + KID_CQ_CAP / 4;   // result slots of a block of 64 reads
    static constexpr uint32_t read_nums = results + 64;            // pair loop: the batch read numbers of 128 result slots
    static constexpr uint32_t total = !MINLOC ? cq_klo : PAIRK ? read_nums + 128 : read_nums;
};
static_assert(KidWaveLds<true, 1>::total == 820 && KidWaveLds<true, 2>::total == 820 && KidWaveLds<true, 0>::total == 792 &&
              KidWaveLds<false, 0>::total == 104, "tests/test_gpu_kernel_variants.py derives the dispatch limits from these");
#define KID_TAPER 6u // the workgroups dispatched first take this many times the reads of those dispatched last
                     // (profiles/r02/ab_taper.txt: a launch ends when the slowest of its last workgroups does)
// A lookup whose header shows a fingerprint match fetches its candidate cell on the spot -- the cell sits in the
// 128-byte line the header has just brought in -- and the queue carries {target, entry ordinal} of verified hits; the
// resolver then needs neither the header nor the cell again (by then the line is long gone from every cache: one HBM
// line and two dependent round trips per hit saved).  Lookups that cannot be settled by their first candidate (a
// fingerprint false positive, a full line) are queued with their key.  Only while hits are sparse:
#define KID_EARLY_MAX 4u // ... tiles with at most this many flagged lookups
#define KID_EARLY_QN 32u // ... while fewer than this many lookups are queued (profiles/r02/clumped_ec.txt)
// Not in the DIGEST instantiations: their hot loop has brought in a plane line, not the table line, so the candidate
// cell would come from HBM, not from L2 behind a header, and waiting for it in the hot loop costs more than deferring
// every flagged lookup: 1138-1160 M pairs/s, with the early path 1091, the header kernels 1089
// (profiles/digest/ab_early_vs_deferred.txt).  The resolver then settles a flagged lookup from its table line alone:
// the header (cell 0, the one HBM request) and the candidate cell behind it in the same 128 bytes -- the digest is not
// read a second time (profiles/resolver_header/).
#define KID_CLASSIFY_OCC 8 // waves per SIMD the register allocator must leave room for
// ... except the duo loop with ancestor rows: at 64 VGPRs it spills, and a spill or copy of a register that an
// asynchronous inline-assembly load (below) has not filled yet carries a stale value past the explicit s_waitcnt --
// wrong hits, found by tests/test_gpu_kernel_variants.py.  Allowed 128 VGPRs it takes 80 (6 waves per SIMD), no spill.
#define KID_CLASSIFY_OCC_DUO_ROWS 4

// ------------------------------------------------------------------ classify
// One wavefront per read (DESIGN.md section 4 has the long version).  What a read needs:
//   1. lane i extracts the k-mer window starting at base i from the read's packed words (16 bases
//      each; general loops: staged in an LDS strip, pair kernels: fetched with ds_bpermute) with
//      two shifts -- no serial rolling --, derives the reverse complement with a bit reversal and
//      takes min(); with the minimizer-localised table the wave also computes the sliding-window
//      minimum of the hashed m-mers (DPP row scans + one cross-lane fetch), which selects the line;
//   2. the table is probed in HBM -- U windows per lane in flight at once.  Minimizer-localised
//      table: one header per lookup, which settles ~99 % of them; the others are queued in LDS and
//      resolved 64 at a time (candidate cell, ancestor row);
//   3. hits are folded with msca in read-position order (the fold is not associative:
//      newkmer_10nx.cpp:588-595);
//   4. hit cells are marked in the sample's seen-bitmap (ucount, :596-603).
// gcount is accumulated in an LDS histogram per workgroup and flushed once.
template <int U, bool DIGEST = false>
struct KidGroup {      // a group of U*64 windows between its two halves
    uint64_t key[U];
    uint32_t hlo[U];   // reference geometry: first cell of the probe sequence; minloc: the table line
    typename std::conditional<DIGEST, uint2, uint4>::type hd[U]; // minloc: header of that line (in flight); DIGEST: its 8-byte digest
    uint32_t fpp;      // minloc: the 16-bit key fingerprints of the U lookups, packed
    bool act[U];
};

// Three instantiations per configuration share this body, picked by the longest read of the batch
// (kid_prepare_kernel leaves it in rare->batch_max): PAIRK = 1 holds the hand-pipelined pair loop for
// batches of single-group reads (<= U*64 k-mers), PAIRK = 2 the same loop with the two groups of one
// read as the pair (<= 2*U*64 k-mers), PAIRK = 0 the general loops.  The host launches the one the
// batch is for when it knows the longest read, else all three: the others return at once.  Separate
// kernels, because each loop wants all 64 vector registers of an 8-waves-per-SIMD kernel for itself.
// DIGEST (pair and duo loops): a lookup reads the 8-byte digest of its line from the plane beside the table instead of
// the line's header (kid_common.h has the layout and why the results are the same).  The table pointer then comes from
// `rare` where a candidate cell or a chained header is fetched, and the plane's takes its scalar registers in the loop.
template <int U, bool ROWS, bool HIST, bool MINLOC, int KFIX, int PAIRK, bool DIGEST = false>
__global__ __launch_bounds__(512, (PAIRK == 2 && ROWS) ? KID_CLASSIFY_OCC_DUO_ROWS : KID_CLASSIFY_OCC) void kid_classify_kernel(const KidDevDb db, const KidInput b, const KidSampleDev s,
                                                            const uint32_t hist_words,
                                                            const KidReadDesc *__restrict__ const descs,
                                                            const KidRareArgs *__restrict__ const rare)
{
    static_assert(!PAIRK || (MINLOC && U == 2), "the pair loop exists for the minimizer-localised table, two windows per lane");
    static_assert(!DIGEST || PAIRK, "the digest plane is read by the pair and duo loops alone");
    typedef KidGroup<U, DIGEST> Group;
    auto cells = [&]() -> const uint4 * { // the table, where a rare path needs it
        if constexpr (DIGEST) return rare->table;
        else return db.table;
    };
    if (MINLOC) { // wave-uniform, before anything else
        const uint32_t longest = (uint32_t)rare->batch_max;
        const int mode = longest <= (uint32_t)(U * 64) ? 1 : longest <= (uint32_t)(2 * U * 64) ? 2 : 0;
        if (mode != PAIRK) return;
    }
    // the launch on the device's own clock (kid_sample_kernel_time_device): first workgroup to start ... last one to end
    if (threadIdx.x == 0) atomicMin(&s.stats[30], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    // (descs == b.desc, passed once more as a restrict-qualified argument: the wave-uniform
    //  descriptor loads then become scalar loads, which stay in flight until first use)
    extern __shared__ uint32_t kid_smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // wave-uniform
    const uint32_t wpb = blockDim.x >> 6;
    uint32_t *hist = kid_smem;
    typedef KidWaveLds<MINLOC, PAIRK> LDS;
    uint32_t *WA = kid_smem + hist_words + wib * LDS::total; // this wave's area

    // the workgroup's totals for kid_sample_stats (behind the waves' areas): one set of global atomics per workgroup --
    // four per WAVE, all on one line, were 32 768 atomics per launch queueing up on one L2 atomic unit (~0.1 ms)
    unsigned long long *const WGS = reinterpret_cast<unsigned long long *>(
        kid_smem + hist_words + wpb * LDS::total);
    if (threadIdx.x < 4) WGS[threadIdx.x] = 0;
    if (HIST) {
        for (uint32_t i = threadIdx.x; i < hist_words; i += blockDim.x) hist[i] = 0;
    }
    __syncthreads();

    const int k = KFIX ? KFIX : db.k; // KFIX = 30: the reference's KSIZE folded into the shifts and masks
    const uint32_t win = (uint32_t)kid_min_window(k); // m-mers per k-mer window: 15, 16 or 17
    const int mlen = kid_min_mlen(k);
    // lane classes of the sliding minimum.  With q = lane mod 16 the window of a lane leaves its 16-lane
    // row iff q + win > 16: then it is min(S[p], P[p+win-1]); inside one row it is the prefix P[p+win-1]
    // alone (q = 0) or the suffix alone (q = 1, win = 15)
    const uint32_t bp_src = ((lane + win - 1u) & 63u) << 2; // ds_bpermute address of lane + win - 1
    const bool p_same = lane + win - 1u < 64u;              // that lane is in the same tile
    const bool p_cross = (lane & 15u) + win > 16u, p_q0 = (lane & 15u) == 0u;
    const uint64_t gw = (uint64_t)blockIdx.x * wpb + wib;
    const uint64_t nw = (uint64_t)gridDim.x * wpb;
    // Counters for kid_sample_stats.  Wave-uniform state that only rare paths touch is kept out of
    // scalar registers (80 per wave at this occupancy, and the hot loop wants them all): lookups and
    // hits accumulate in the wave's LDS words, the msca row of the running result in lanes 0-3 of a
    // vector register, the probes beyond the first in a per-lane counter.
    uint32_t *const WC = WA + LDS::counters; // [0..1] lookups (64 bits), [2] hits, [3] probes beyond the first of a lookup
    unsigned long long *const WL = reinterpret_cast<unsigned long long *>(WC);
    if (lane < 4) WC[lane] = 0;
    uint32_t pend_t = 0, pend_n = 0;       // !HIST: run-length buffer in front of the global gcount atomics

    // ---- 1. stage one packed segment in a strip; returns "no base of it resets a window" (wave-uniform)
    auto stage = [&](uint32_t *W, const uint32_t codes, const uint32_t inv) -> bool {
        uint32_t *IM = W + (LDS::mask - LDS::strip);
        W[lane] = codes;
        reinterpret_cast<uint16_t *>(IM)[lane] = (uint16_t)inv;
        if (lane < 2) { W[64 + lane] = 0; IM[32 + lane] = 0; }
        const bool clean = (__ballot(inv != 0) == 0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        return clean;
    };

    // ---- 2, 3a. windows [t0, t0 + U*64) of the staged segment: keys, table line, header loads issued
    auto group_front = [&](const uint32_t *W, const uint32_t sh, const uint32_t nb, const uint32_t segk, const uint32_t t0,
                           const bool seg_clean, Group &g, uint32_t &n_bad, const bool issue_loads = true,
                           const uint32_t wcodes = 0, const uint32_t winv = 0) {
        // W == nullptr (pair kernels): no LDS strip; the lanes hold the read's packed words and masks in (wcodes, winv)
        // -- word c of the read in the LW = 4 (pair kernel) or 2 (duo kernel) lanes that loaded its 16 bases, see
        // pack_lanes -- and a window fetches its three words with ds_bpermute: one LDS round trip instead of
        // write + barrier + read.  Needs the whole read inside 64 / LW words, which one (two) group(s) of a read are.
        const bool direct = (W == nullptr);
        constexpr uint32_t LWS = PAIRK == 1 ? 2u : 1u; // log2 of the lanes per word
        auto word = [&](const uint32_t idx) -> uint32_t {
            return direct ? (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << (2u + LWS)), (int)wcodes) : W[idx];
        };
        auto mask32 = [&](const uint32_t idx) -> uint32_t { // invalid-mask bits of bases 32 idx .. 32 idx + 31
            if (!direct) return (W + (LDS::mask - LDS::strip))[idx];
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << (3u + LWS)), (int)winv);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((idx << (3u + LWS)) + (4u << LWS)), (int)winv);
            return (lo & 0xFFFFu) | (hi << 16);
        };
        uint32_t P[U + 1], S[U]; // minloc: row prefix / suffix minima of the hashed m-mers
        const uint32_t pmax = sh + nb - (uint32_t)mlen; // last m-mer start inside the segment
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = t0 + (uint32_t)u * 64u + lane;
            // one window extraction serves the k-mer AND the m-mer that starts at the same base;
            // lanes past the last k-mer still hash their m-mer (the windows of earlier lanes reach
            // 14 positions ahead), clamped to the last one that lies inside the segment
            uint32_t p = sh + i;
            p = MINLOC ? (p < pmax ? p : pmax) : sh + (i < segk ? i : 0u);
            const uint32_t w0 = p >> 4, o2 = (p & 15u) * 2u;
            const uint64_t A = ((uint64_t)word(w0) << 32) | word(w0 + 1);
            const uint64_t B = word(w0 + 2);
            const uint64_t x = (A << o2) | ((B << o2) >> 32);
            const uint64_t keyF = x >> (64 - 2 * k);
            // one reversal of the 32-base window serves both reverse complements: base j of the window
            // lands in bits [2j+1, 2j], so the low 2k bits are the k-mer's and the low 2m bits the m-mer's
            const uint64_t nrv = ~kid_rev2(x);
            const uint64_t keyR = nrv & (~0ull >> (64 - 2 * k));
            bool valid = (i < segk);
            if (!seg_clean) { // rare: some base of the segment is not ACGTacgt
                const uint64_t im = (((uint64_t)mask32((p >> 5) + 1) << 32) | mask32(p >> 5)) >> (p & 31u);
                const bool ok = ((im & ((1ull << k) - 1ull)) == 0);
                n_bad += (uint32_t)__popcll(__ballot(valid && !ok));
                valid = valid && ok;
            }
            g.key[u] = keyF < keyR ? keyF : keyR; // newkmer_10nx.cpp:528
            if (!MINLOC) g.hlo[u] = (uint32_t)kid_fmix64(g.key[u]) & db.slot_mask;
            g.act[u] = valid;
            if (MINLOC) {
                const uint32_t h = kid_mmer_hash2((uint32_t)(x >> (64 - 2 * mlen)), (uint32_t)nrv & (0xFFFFFFFFu >> (32 - 2 * mlen)));
                P[u] = h;
                S[u] = h;
            }
        }
        if (MINLOC) {
            if constexpr (U == 2) kid_row_scans(P[0], S[0], P[1], S[1]);
            else {
#pragma unroll
                for (int u = 0; u < U; u++) { P[u] = kid_row_prefix_min(P[u]); S[u] = kid_row_suffix_min(S[u]); }
            }
        }
        if (MINLOC) {
            g.fpp = 0;
#pragma unroll
            for (int u = 0; u < U; u++) g.fpp |= kid_key_fp(g.key[u]) << (16 * u);
            // the win-1 m-mers behind the last k-mer of the group -- if any window of the group reaches that
            // far (wave-uniform: a 100-bp read ends inside the group, m-mers and all)
            P[U] = 0xFFFFFFFFu;
            if (segk + win - 1u > t0 + (uint32_t)U * 64u) {
                uint32_t p = sh + t0 + (uint32_t)U * 64u + lane;
                p = p < pmax ? p : pmax;
                const uint32_t w0 = p >> 4, o2 = (p & 15u) * 2u;
                const uint64_t A = ((uint64_t)word(w0) << 32) | word(w0 + 1);
                P[U] = kid_row_prefix_min(kid_mmer_hash((uint32_t)((A << o2) >> (64 - 2 * mlen)), mlen));
            }
            // ... and their minimum over every window a[p..p+win-1].  With q = p mod 16: the window
            // leaves its 16-lane row iff q + win > 16, then it is min(S[p], P[p+win-1]); inside
            // one row it is exactly the prefix P[p+win-1] (q = 0) or the suffix S[p] (win = 15, q = 1)
            uint32_t nxt = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bp_src, (int)P[0]);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t same = nxt;
                nxt = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bp_src, (int)P[u + 1]);
                const uint32_t pn = p_same ? same : nxt;
                const uint32_t both = S[u] < pn ? S[u] : pn;
                const uint32_t mz = p_cross ? both : (p_q0 ? pn : S[u]);
                // one 16-byte header per lookup settles every absent key; lanes that share a
                // minimizer read the same header (one sector for all of them)
                g.hlo[u] = kid_minloc_line(mz, db.line_shift);
                if constexpr (DIGEST) g.hd[u] = make_uint2(0, 0); // (the pair and duo loops issue their loads themselves)
                else {
                    g.hd[u] = make_uint4(0, 0, 0, 0);
                    if (issue_loads && g.act[u]) g.hd[u] = kid_load_cell(db.table, g.hlo[u] * KID_LINE_CELLS);
                }
            }
        }
    };

    // ---- 3b, 4, 5. the rest of the probe sequences, seen-bitmap, ordered fold into final_t (vfrow:
    // the ancestor row of final_t, in lanes 0-3)
    auto group_back = [&](auto &g, uint32_t &final_t, uint32_t &vfrow) {
        static_assert(!MINLOC && sizeof(g) != 0, "the minimizer-localised table has no back half on the spot");
        uint32_t tgt[U], slot[U];
#pragma unroll
        for (int u = 0; u < U; u++) { tgt[u] = 0; slot[u] = 0; }
        {
            uint64_t rp[U];
            uint32_t step[U];
#pragma unroll
            for (int u = 0; u < U; u++) { rp[u] = 0; step[u] = 0; }
            bool any = false;
#pragma unroll
            for (int u = 0; u < U; u++) any |= g.act[u];
            while (any) {
                uint4 c[U];
                uint32_t idx[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    idx[u] = (g.hlo[u] + (uint32_t)rp[u]) & db.slot_mask;
                    c[u] = make_uint4(0, 0, 0, 0);
                    if (g.act[u]) c[u] = kid_load_cell_nt(db.table, idx[u]);
                }
                any = false;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (g.act[u]) {
                        step[u]++;
                        rp[u] += step[u];
                        if (step[u] > 1) atomicAdd(&WC[3], 1u);
                        if (c[u].z == 0) g.act[u] = false;
                        else if (c[u].x == (uint32_t)g.key[u] && c[u].y == (uint32_t)(g.key[u] >> 32)) {
                            tgt[u] = c[u].z; slot[u] = c[u].w - 1u; g.act[u] = false;
                        } else if (!(rp[u] < db.nslots) || (db.max_probes != 0 && step[u] >= db.max_probes)) g.act[u] = false;
                    }
                    any |= g.act[u];
                }
            }
        }
        uint4 row[U];
        uint64_t hitm[U];
        uint32_t nh = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            row[u] = make_uint4(0, 0, 0, 0);
            if (tgt[u] > 0) {
                if (ROWS) row[u] = db.rows[tgt[u]];
                if (tgt[u] > 1) kid_atomic_or_nowait(&s.seen[slot[u] >> 5], 1u << (slot[u] & 31u));
            }
            hitm[u] = __ballot(tgt[u] > 0);
            nh += (uint32_t)__popcll(hitm[u]);
        }
        if (nh == 0) return;
        if (lane == 0) atomicAdd(&WC[2], nh);
#pragma unroll
        for (int u = 0; u < U; u++) {
            uint64_t m = hitm[u];
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)tgt[u], j);
                if (x == final_t) continue; // msca(x,x) = x
                uint4 rx = make_uint4(0, 0, 0, 0);
                if (ROWS) rx = kid_row_of_lane(row[u], j);
                if (final_t != 0) { // :588-591
                    if (ROWS) {
                        uint4 ro;
                        final_t = kid_msca_rows(x, rx, final_t, kid_row_unpack(vfrow), ro);
                        rx = ro;
                    } else {
                        final_t = kid_msca_climb(db, x, final_t);
                    }
                } else {
                    final_t = x; // :592-595
                }
                if (ROWS)
                    vfrow = lane == 0 ? rx.x : lane == 1 ? rx.y : lane == 2 ? rx.z : lane == 3 ? rx.w : vfrow;
            }
        }
    };

    // ---- gcount[final]++ (:605) and the per-read output
    auto finish_read = [&](const uint64_t r, const uint32_t final_t, const uint32_t n_valid) {
        if (HIST) {
            if (lane == 0) { atomicAdd(&hist[final_t], 1u); atomicAdd(WL, (unsigned long long)n_valid); }
        } else {
            if (lane == 0) atomicAdd(WL, (unsigned long long)n_valid);
            if (final_t == pend_t) {
                pend_n++;
            } else {
                if (pend_n && lane == 0) atomicAdd(&rare->gcount[pend_t], (unsigned long long)pend_n);
                pend_t = final_t;
                pend_n = 1;
            }
        }
        if (lane == 0 && b.out_final) kid_store_u32_nowait(&b.out_final[r], final_t);
    };

    // ==== minimizer-localised table: the back half is deferred (both kernels) =======================
    // ---- back half, deferred.  A lookup whose header shows a fingerprint match (or a chained line)
    // is not followed up on the spot -- that would put two more dependent round trips (hit cell,
    // ancestor row) on every second read -- but queued in LDS; queued lookups are resolved 64 at a
    // time, one per lane, and folded read by read (entries are in read order, then window order).
    uint32_t *const CQ_klo = WA + LDS::cq_klo, *const CQ_khi = WA + LDS::cq_khi, *const CQ_lw = WA + LDS::cq_lw;
    uint8_t *const CQ_tag = reinterpret_cast<uint8_t *>(WA + LDS::cq_tag); // read number mod 64
    // per-read results wait in LDS for one scattered store per 64 reads: a pending store shares vmcnt
    // with the loads, and the explicit counts of the loop would have to sit out its acknowledgement
    uint32_t *const RB = WA + LDS::results;
    const uint32_t gw32 = (uint32_t)gw, nw32 = (uint32_t)nw; // 32-bit read indices (n < 2^31): read number i of this wave is gw + i nw
    uint32_t rd_first = gw32, rd_stride = nw32; // ... except where a wave takes a contiguous range (set below): rd_first + i
    uint32_t gen_cnt = 0;                         // general loops: reads of this wave
    uint64_t rb_skip = 0;   // result slots of the current block of 64 reads that are not this pass's to store
    bool rb_direct = false; // second pass of the general loops (reads of more than one segment): results stored at once
    uint32_t *const RG = WA + LDS::read_nums; // pair kernel: which read of the batch a result slot belongs to (128 slots: the next block's are known early)
    auto flush_results = [&](const uint32_t i0, const uint32_t n) { // this wave's reads i0 .. i0+n-1 (n <= 64)
        uint32_t *const outp = rare->out_final;
        if (outp && lane < n && !((rb_skip >> ((i0 + lane) & 63u)) & 1ull))
            kid_store_u32_nowait(&outp[PAIRK == 1 ? RG[(i0 + lane) & 127u] : rd_first + (i0 + lane) * rd_stride], RB[(i0 + lane) & 63u]);
        rb_skip = 0;
        RB[lane] = 0; // (a read without any hit does not write its slot: see commit_zero)
    };
    if (MINLOC) RB[lane] = 0;
    uint32_t n_zero = 0;    // wave-uniform: reads classified as 0 that have not been added to gcount[0] yet
    uint32_t qn = 0;        // wave-uniform fill of the queue
    uint32_t n_lookups = 0; // wave-uniform; per wave and launch: stays below 2^32 for batches of < 2^31 reads x 128 k-mers (longer reads: mod 2^32 is accepted for this counter)
    // the read the resolver left open (its run ended a chunk, or it is still being classified), and its fold so far
    uint32_t cur_tag = 0xFFFFFFFFu, final_c = 0, vfrow_c = 0;
    // what a finished read leaves, by the lane that knows its result f: gcount[f]++ (:605) in the workgroup's histogram
    // (without one: the caller's own way to gcount), and the result stored at once or slotted for the flush
    auto count_hist = [&](const uint32_t f) { atomicAdd(&hist[f >> 1], 1u << (16u * (f & 1u))); };
    auto put_result = [&](const uint32_t i, const uint32_t f) { // i: the read's number in this wave
        if (rb_direct) { if (b.out_final) kid_store_u32_nowait(&b.out_final[rd_first + i * rd_stride], f); }
        else RB[i & 63u] = f;
    };
    auto commit = [&](const uint32_t i, const uint32_t final_t) {
        if (HIST) {
            if (lane == 0) count_hist(final_t);
        } else if (final_t == pend_t) {
            pend_n++;
        } else {
            if (pend_n && lane == 0) atomicAdd(&rare->gcount[pend_t], (unsigned long long)pend_n);
            pend_t = final_t;
            pend_n = 1;
        }
        if (lane == 0) put_result(i, final_t);
    };
    // the common case, a read without a single candidate: counted in a scalar register, its result slot is
    // zero already
    auto commit_zero = [&](const uint32_t i) {
        n_zero++;
        if (rb_direct && lane == 0 && b.out_final) kid_store_u32_nowait(&b.out_final[rd_first + i * rd_stride], 0u);
    };
    // i_now: number of the newest queued read (all are within 63 of it); open_tag: a read that may still get
    // entries (general loops, between the groups of a read) -- its run is folded but not committed
    // (always inlined: left as a call -- the duo loop with rows and without a histogram sits at the inliner's threshold --
    //  the groups it is handed live in scratch and the loop's scalars in vector registers)
    auto resolve_all = [&](const uint32_t i_now, const uint32_t open_tag) __attribute__((always_inline)) {
        // (the pair kernel never leaves a read open between calls: its carry lives and dies in here)
        uint32_t ctag = PAIRK == 1 ? 0xFFFFFFFFu : cur_tag, final_t = PAIRK == 1 ? 0u : final_c, vfrow = PAIRK == 1 ? 0u : vfrow_c;
        auto commit_tag = [&](const uint32_t tag, const uint32_t f) {
            commit(i_now - ((i_now - tag) & 63u), f);
        };
        for (uint32_t base = 0; base < qn; base += 64u) {
            const uint32_t n = qn - base < 64u ? qn - base : 64u;
            const bool valid = lane < n;
            // places in the hit log for this chunk: asked for now, looked at when the targets are known
            uint32_t *const slog = rare->seen_log;
            uint32_t log_at = 0;
            if (slog && lane == 0) log_at = atomicAdd(rare->seen_log_tail + (blockIdx.x & (KID_LOG_SHARDS - 1u)) * 16u, n);
            uint32_t klo = 0, khi = 0, ln = 0, tag = 0;
            if (valid) { klo = CQ_klo[base + lane]; khi = CQ_khi[base + lane]; ln = CQ_lw[base + lane]; tag = CQ_tag[base + lane]; }
            const bool verified = (tag & 0x80u) != 0; // {target, entry ordinal} fetched when the header came in
            tag &= 63u;
            // the header (the queue keeps only the line: working out the candidates at queueing time would cost the hot
            // loop ~45 instructions per read with a match).  Header kernels: once more, usually still in L2.  DIGEST: for
            // the first time -- the hot loop flagged the lookup on the digest's 8-bit fingerprints, and the header's 16-bit
            // ones, count and 12-bit filter decide here; it arrives with the 128-byte line the candidate cell lies in, so a
            // flagged lookup costs one table line, and a false flag of the digest no cell load at all
            uint32_t tgt = 0, slot = 0, mu = 0;
            const uint32_t fp = kid_key_fp(((uint64_t)khi << 32) | klo);
            bool fu = false;
            if (verified) { tgt = klo; slot = khi; }
            if (valid && !verified) {
                const uint4 h = kid_load_cell(cells(), ln * KID_LINE_CELLS);
                mu = kid_hdr_cand(h, fp);
                fu = kid_hdr_continues(h.w, fp);
            }
            { // (cells read: one add for the wave, not one per lane on the same LDS word)
                const uint64_t cm = __ballot(mu != 0);
                if (cm && lane == 0) atomicAdd(&WC[3], (uint32_t)__popcll(cm));
            }
            if (mu) { // the first candidate of every entry in one round trip: almost always the key itself
                const uint32_t bit = (uint32_t)__builtin_ctz(mu);
                const uint32_t idx = ln * KID_LINE_CELLS + 1u + kid_cand_entry(bit);
                mu &= mu - 1;
                const uint4 c = kid_load_cell(cells(), idx);
                if (c.z != 0 && c.x == klo && c.y == khi) { tgt = c.z; slot = c.w - 1u; }
            }
            bool go = valid && !verified && tgt == 0 && (mu != 0 || fu);
            while (go) { // a second candidate (1e-4 of the lookups) or a chained line (1e-5)
                if (mu) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(mu);
                    const uint32_t j = kid_cand_entry(bit);
                    mu &= mu - 1;
                    const uint32_t ix = ln * KID_LINE_CELLS + 1u + j;
                    const uint4 cc = kid_load_cell(cells(), ix);
                    atomicAdd(&WC[3], 1u);
                    if (cc.z != 0 && cc.x == klo && cc.y == khi) { tgt = cc.z; slot = cc.w - 1u; go = false; }
                } else if (fu) { // (a chain is followed along the table's headers, with or without a digest: a 1e-5 event)
                    ln = (ln + 1u) & rare->line_mask;
                    const uint4 h = kid_load_cell(cells(), ln * KID_LINE_CELLS);
                    atomicAdd(&WC[3], 1u);
                    mu = kid_hdr_cand(h, fp);
                    fu = kid_hdr_continues(h.w, fp);
                } else go = false;
            }
            uint4 row = make_uint4(0, 0, 0, 0);
            if (tgt > 0) {
                if (ROWS) row = rare->rows[tgt];
            }
            {
                // kmer_seen (:596-600).  The entries of a pass are in read and window order, and consecutive k-mers of a
                // genome carry consecutive entry ordinals when the database lists them in genome order (the reference's
                // builder does): the hits of a read then fall into two or three words of the bitmap.  Lanes that name the
                // same word as a lane 1, 2, 4 or 8 places before them in their 16-lane row take that lane's bits along
                // (bits of the same word, set by hits of this pass: OR-ing them in once more is harmless), and only the
                // last lane of a run issues the atomic.  60 hits per read: 121 M atomics per 2 M reads became 1/16 of
                // that; each one occupies an L2 channel for ~16 cycles (profiles/r02/ab_hitlog.txt).
                const bool sb = tgt > 1;
                // The log: one coalesced store per chunk instead of one memory-side atomic per hit -- 2.5 M of those per
                // 1 M read pairs, each worth several line fetches of channel time (8-10 % of the launch,
                // profiles/r03/ab_noseen.txt).  kid_seenlog_* sets the bits later, a bitmap piece at a time in LDS.
                bool logged = false;
                if (slog) {
                    const uint32_t cap = rare->seen_log_cap;
                    const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)log_at);
                    uint32_t *const at_p = slog + (size_t)(blockIdx.x & (KID_LOG_SHARDS - 1u)) * cap + at;
                    if (at <= cap - n) { // (cap >= 64)
                        if (valid) kid_store_u32_nowait(at_p + lane, sb ? slot : KID_LOG_NONE);
                        logged = true;
                    } else if (at < cap && lane < cap - at) {
                        // the region is full: back to atomics until the log has been applied -- but the places that were
                        // handed out up to its end must not be left as they are (the pass reads everything below the end)
                        kid_store_u32_nowait(at_p + lane, KID_LOG_NONE);
                    }
                }
                if (!logged) {
                const uint32_t word = sb ? slot >> 5 : 0xFFFFFFF0u + (lane & 15u); // (no two neighbours without a hit alike)
                uint32_t bits = sb ? 1u << (slot & 31u) : 0u;
#define KID_SEEN_STEP(CTRL)                                                                                                    \
                {                                                                                                               \
                    const uint32_t w_ = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)word, CTRL, 0xF, 0xF, false); \
                    const uint32_t b_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, CTRL, 0xF, 0xF, false);               \
                    if (w_ == word) bits |= b_;                                                                                 \
                }
                KID_SEEN_STEP(0x111) KID_SEEN_STEP(0x112) KID_SEEN_STEP(0x114) KID_SEEN_STEP(0x118) // row_shr:1, 2, 4, 8
#undef KID_SEEN_STEP
                const uint32_t w_next = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)word, 0x101, 0xF, 0xF, false); // row_shl:1
                if (sb && w_next != word) kid_atomic_or_nowait(&rare->seen[word], bits);
                }
            }
            const uint64_t hitm = __ballot(tgt > 0);
            if (hitm && lane == 0) atomicAdd(&WC[2], (uint32_t)__popcll(hitm));
            // Fold read by read, one lane per read: entries of a read are neighbours (a change of tag
            // starts the next read); the first lane of a run walks its run in window order, fetching
            // (target, ancestor row) of entry lane + t with ds_bpermute.  The left fold of msca over
            // the hits of a read, newkmer_10nx.cpp:588-595.
            const uint32_t tprev = (uint32_t)__shfl_up((int)tag, 1);
            const bool head = valid && (lane == 0 || tag != tprev);
            const uint64_t hm = __ballot(head);
            const uint64_t above = lane < 63u ? (hm >> (lane + 1u)) : 0ull;
            const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) + 1u : n - lane; // entries of this run (head lanes)
            uint32_t f = 0;
            uint4 fr = make_uint4(0, 0, 0, 0);
            if (lane == 0 && ctag != 0xFFFFFFFFu) {
                if (valid && tag == ctag) { // the run continues the read left open by the chunk before
                    f = final_t;
                    fr = kid_row_unpack(vfrow);
                }
            }
            if (ctag != 0xFFFFFFFFu && (uint32_t)__builtin_amdgcn_readfirstlane((int)tag) != ctag) commit_tag(ctag, final_t);
            if (__popcll(hm) <= 6) {
                // Few, long runs (reads with many hits): the runs in turn, all entries of a run at once.
                // Every lane works out the step its own entry would make from the run's current result;
                // entries up to the first one that changes the result leave it as it is -- which is all
                // the sequential fold would have done with them -- so the run jumps there and repeats.
                // One round per change of the result, a handful per read, instead of one per hit.
                uint64_t runs = hm;
                while (runs) {
                    const int h = __builtin_ctzll(runs);
                    runs &= runs - 1;
                    const uint32_t e = runs ? (uint32_t)__builtin_ctzll(runs) : n; // the run is [h, e)
                    uint32_t uf = (uint32_t)__builtin_amdgcn_readlane((int)f, h);
                    uint4 ufr = kid_row_of_lane(fr, h);
                    uint64_t rem = hitm & (e >= 64u ? ~0ull : ((1ull << e) - 1ull)) & ~((1ull << h) - 1ull);
                    while (rem) { // (kid_jump_fold of kid_tile.hip.h, written out on this loop's registers)
                        uint32_t rj = tgt;
                        uint4 roj = row;
                        if (uf != 0 && tgt != uf) { // (first hit: :592-595; msca(x,x) = x)
                            if (ROWS) rj = kid_msca_rows(tgt, row, uf, ufr, roj);
                            else rj = kid_msca_climb(db, tgt > 0 ? tgt : uf, uf);
                        }
                        const uint64_t ch = __ballot(rj != uf) & rem;
                        if (!ch) break;
                        const int j = __builtin_ctzll(ch);
                        uf = (uint32_t)__builtin_amdgcn_readlane((int)rj, j);
                        ufr = kid_row_of_lane(roj, j);
                        rem &= j >= 63 ? 0ull : ~((2ull << j) - 1ull);
                    }
                    if (lane == (uint32_t)h) { f = uf; fr = ufr; }
                }
            } else
            for (uint32_t t = 0; __ballot(head && t < len) != 0; t++) {
                const int src = (int)(((lane + t) & 63u) << 2);
                const uint32_t x = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tgt);
                const uint4 rx = kid_row_bpermute(src, row);
                if (head && t < len && x != 0 && x != f) { // msca(x,x) = x
                    if (f != 0) {
                        if (ROWS) {
                            uint4 ro;
                            f = kid_msca_rows(x, rx, f, fr, ro);
                            fr = ro;
                        } else {
                            f = kid_msca_climb(db, x, f);
                        }
                    } else {
                        f = x; // :592-595
                        fr = rx;
                    }
                }
            }
            // every run but the last one is a finished read; the last one too unless a chunk follows
            const uint32_t last = 63u - (uint32_t)__builtin_clzll(hm); // hm != 0: n >= 1
            const bool more_chunks = base + 64u < qn || (uint32_t)__builtin_amdgcn_readlane((int)tag, (int)last) == open_tag; // "keep the last run open"
            if (head && (lane != last || !more_chunks)) {
                if (HIST) count_hist(f);
                else atomicAdd(&rare->gcount[f], 1ull);
                put_result(i_now - ((i_now - tag) & 63u), f); // (tag = read number mod 64)
            }
            if (more_chunks) {
                ctag = (uint32_t)__builtin_amdgcn_readlane((int)tag, (int)last);
                final_t = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)last);
                const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)fr.x, (int)last), a1 = (uint32_t)__builtin_amdgcn_readlane((int)fr.y, (int)last);
                const uint32_t a2 = (uint32_t)__builtin_amdgcn_readlane((int)fr.z, (int)last), a3 = (uint32_t)__builtin_amdgcn_readlane((int)fr.w, (int)last);
                vfrow = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : lane == 3 ? a3 : vfrow;
            } else {
                ctag = 0xFFFFFFFFu;
            }
        }
        if (ctag != 0xFFFFFFFFu && ctag != open_tag) { commit_tag(ctag, final_t); ctag = 0xFFFFFFFFu; }
        if (PAIRK != 1) { cur_tag = ctag; final_c = final_t; vfrow_c = vfrow; }
        qn = 0;
        // a real s_waitcnt (not inline assembly): hipcc's waitcnt pass then knows that none of ITS loads is
        // pending when this rare path rejoins the loop, and does not drain vmcnt at the top of every trip
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0), expcnt and lgkmcnt untouched
    };
    // header test of one group of a read; its unsettled lookups go to the queue.  false: there were none
    auto back_deferred = [&](const Group &g, const uint32_t i) -> bool {
        uint32_t fp[U];
        bool mm[U], more = false;
#pragma unroll
        for (int u = 0; u < U; u++) {
            fp[u] = (g.fpp >> (16 * u)) & 0xFFFFu;
            // (a full line: word 3 >= 8 << 16 -- filter bits are only ever set on full lines.  Whether THIS key was
            //  pushed past it is looked at by the resolver: testing the filter bit here costs the hot loop a register)
            if constexpr (DIGEST) mm[u] = g.act[u] && (kid_digest_cand(g.hd[u].x, g.hd[u].y, fp[u]) != 0 || kid_digest_count(g.hd[u].y) >= KID_HDR_FULL);
            else mm[u] = g.act[u] && (kid_hdr_any(g.hd[u], fp[u]) || (g.hd[u].w >> 16) >= KID_HDR_FULL);
            more |= mm[u];
        }
        if (__ballot(more) == 0) return false; // (wave-uniform) ~99 % of the lookups are settled by their header
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t qm = __ballot(mm[u]);
            if (qm == 0) continue;
            // (only while hits are sparse: with many flagged lookups per tile the resolver runs every few reads, finds the
            //  lines still in the L2, and the wait for the candidate here would cost more than its second fetch --
            //  builder-shaped database, 15.9 hits per read: 2.15 vs 1.92 ms per 1 M pairs, profiles/r02/clumped_ec.txt)
            const bool early = !DIGEST && (uint32_t)__popcll(qm) <= KID_EARLY_MAX && qn < KID_EARLY_QN;
            uint32_t cm = 0;
            if constexpr (!DIGEST) cm = (early && mm[u]) ? kid_hdr_cand(g.hd[u], fp[u]) : 0u;
            { // (cells read: one add for the wave)
                const uint64_t cmb = __ballot(cm != 0);
                if (cmb && lane == 0) atomicAdd(&WC[3], (uint32_t)__popcll(cmb));
            }
            if (mm[u]) {
                const uint32_t pos = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(qm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qm, 0u));
                uint32_t w0 = (uint32_t)g.key[u], w1 = (uint32_t)(g.key[u] >> 32), tagv = i & 63u;
                if (cm) { // the first candidate, while its line is in the cache
                    const uint32_t idx = g.hlo[u] * KID_LINE_CELLS + 1u + kid_cand_entry((uint32_t)__builtin_ctz(cm));
                    const uint4 c = kid_load_cell(db.table, idx);
                    if (c.z != 0 && c.x == w0 && c.y == w1) { w0 = c.z; w1 = c.w - 1u; tagv |= 0x80u; } // verified: {target, ordinal}
                }
                CQ_klo[pos] = w0;
                CQ_khi[pos] = w1;
                CQ_lw[pos] = g.hlo[u];
                CQ_tag[pos] = (uint8_t)tagv;
            }
            qn += (uint32_t)__popcll(qm);
        }
        return true;
    };

    // ---- the read driver of the general loops.  A read between its segments:
    struct Read {
        bool prefetched = false, had = false; // `prefetch` has been called; some lookup of the read was queued
        uint32_t final_t = 0, vfrow = 0;      // reference geometry: the fold so far, and its ancestor row in lanes 0-3
        uint32_t n_bad = 0;                   // windows without a k-mer
    };
    // one segment (<= KID_SEG_KMERS k-mers behind a shift of sh bases, its text in `raw`): staged, then group by group.
    // `prefetch` issues the loads for the reads behind this one; it is called right after this read's first header
    // loads went out (not before the loops: the compiler drains vmcnt in front of a loop)
    auto run_segment = [&](Read &rd, const uint32_t i, const uint32_t sh, const uint32_t segk, const kid_u4 raw, auto &&prefetch) {
        const uint32_t nb = segk + (uint32_t)k - 1;
        uint32_t codes, inv;
        kid_pack16(make_uint4(raw.x, raw.y, raw.z, raw.w), db.u_is_t, codes, inv);
        const bool seg_clean = stage(WA + LDS::strip, codes, inv);
        for (uint32_t t0 = 0; t0 < segk; t0 += U * 64u) {
            Group g;
            group_front(WA + LDS::strip, sh, nb, segk, t0, seg_clean, g, rd.n_bad);
            if (!rd.prefetched) { prefetch(); rd.prefetched = true; }
            if constexpr (MINLOC) {
                rd.had |= back_deferred(g, i);
                if (qn >= KID_CQ_FLUSH) resolve_all(i, i & 63u); // the read stays open: more groups may follow
            } else {
                group_back(g, rd.final_t, rd.vfrow);
            }
        }
        __builtin_amdgcn_wave_barrier(); // strip is rewritten by the next segment / read
    };
    auto close_read = [&](Read &rd, const uint64_t r, const uint32_t i, const uint32_t n_kmers, auto &&prefetch) {
        if constexpr (MINLOC) {
            n_lookups += n_kmers - rd.n_bad;
            if (!rd.had) commit_zero(i); // (else the resolver commits it, now that it is closed)
        } else {
            finish_read(r, rd.final_t, n_kmers - rd.n_bad);
        }
        if (!rd.prefetched) prefetch();
    };
    // a whole read of any length on its own, given its descriptor and the text of its first segment
    auto process_read = [&](const uint64_t r, const uint32_t i, const uint64_t first, const int64_t nk, const kid_u4 st_raw,
                            auto &&prefetch) {
        Read rd;
        for (int64_t seg = 0; seg < nk; seg += KID_SEG_KMERS) {
            const uint32_t segk = (uint32_t)((nk - seg) < KID_SEG_KMERS ? (nk - seg) : KID_SEG_KMERS);
            const uint64_t b0 = first + (uint64_t)seg; // first base of the segment
            const uint32_t sh = (uint32_t)(b0 & 15ull);
            const uint32_t nchunks = (sh + segk + (uint32_t)k - 1 + 15u) >> 4; // <= 64
            kid_u4 raw = st_raw;
            if (seg != 0) // long reads: later segments are fetched on the spot (lanes past the segment: its first chunk again)
                raw = *reinterpret_cast<const kid_u4 *>(b.bases + 16ull * ((b0 >> 4) + (lane < nchunks ? lane : 0u)));
            run_segment(rd, i, sh, segk, raw, prefetch);
        }
        close_read(rd, r, i, nk > 0 ? (uint32_t)nk : 0u, prefetch);
    };

    auto fetch_desc = [&](uint32_t r, KidReadDesc &d) {
        d.first_base = 0; d.n_kmers = 0; d.pad = 0;
        if (r < (uint32_t)b.n) {
            if (b.desc) d = descs[r];
            else { d.first_base = (rare->read0 + r) * (unsigned long long)rare->fixed_len; d.n_kmers = rare->fixed_nk; } // fixed layout
        }
    };
    // the first segment of a read as text: lane c asks for the 16 bytes of chunk c.  Unconditional -- a fixed number of
    // loads keeps the compiler's vmcnt bookkeeping exact, so the waits for older loads do not drain these -- but never
    // beyond the chunk that holds the segment's last base: the lanes past it ask for its first chunk again (their words
    // are never looked at).  Wave-uniform base + 32-bit lane offset: the scalar-base addressing form
    auto fetch_words = [&](const KidReadDesc &d, kid_u4 &raw) {
        const uint32_t segk = d.n_kmers > KID_SEG_KMERS ? (uint32_t)KID_SEG_KMERS : d.n_kmers > 0 ? (uint32_t)d.n_kmers : 0u;
        const uint32_t nchunks = (((uint32_t)d.first_base & 15u) + segk + (uint32_t)k - 1u + 15u) >> 4;
        raw = *reinterpret_cast<const kid_u4 *>(reinterpret_cast<const char *>(b.bases + 16ull * (d.first_base >> 4)) + (lane < nchunks ? lane : 0u) * 16u);
    };
    auto uniform64 = [](uint64_t v) {
        return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    };
    // ---- phase 1: every read of one segment (<= 960 k-mers: all short-read data).  Longer ones are
    // left to phase 2, so that their loop nest and 64-bit bookkeeping stay out of this loop's registers
    bool any_long = false;
    auto short_read = [&](const uint32_t r, const uint32_t i, const uint64_t first, const int32_t nk, const kid_u4 st_raw,
                          auto &&prefetch) {
        if (nk > KID_SEG_KMERS) { any_long = true; rb_skip |= 1ull << (i & 63u); prefetch(); return; }
        Read rd;
        if (nk > 0) run_segment(rd, i, (uint32_t)first & 15u, (uint32_t)nk, st_raw, prefetch);
        close_read(rd, r, i, nk > 0 ? (uint32_t)nk : 0u, prefetch);
    };
    uint32_t reads_done = gw < b.n ? (uint32_t)((b.n - gw + nw - 1) / nw) : 0u; // the wave's strided share (the pair kernel counts its own)
    // ---- batches whose reads all fit one group (<= U*64 k-mers: Illumina reads): hand-pipelined pairs.
    // A wave is a chain of dependent round trips (strip, header, hit cell, ancestor row) that eight waves
    // per SIMD do not cover, so two reads travel together: front half of A, front half of B (four header
    // loads per lane in flight), the packed words of the next pair, then the back halves.  The compiler's
    // waitcnt insertion drains vmcnt(0) whenever loads sit behind a branch or a store is pending, which
    // serialises exactly these round trips; the loads of this loop are therefore issued from inline
    // assembly, unconditionally (idle lanes read cell 0), and waited for with explicit counts.  Loads
    // return in order, and anything the compiler issues in between (hit cells, atomics, the out_final
    // store) only makes an explicit count stricter than needed.
    if constexpr (PAIRK != 0) {
        uint32_t cnt = 0, duo_first = 0; // duo kernel: the wave's reads are duo_first .. duo_first + cnt - 1
        if (PAIRK == 2) {
            // the duo kernel's waves take one contiguous range of reads each, in the pair kernel's shrinking shares (see
            // switch_block): KID_TAPER units of reads per wave in the first half of the workgroups, one in the second
            const uint32_t nb2 = (uint32_t)b.n, G = gridDim.x, half = G >> 1, wg = blockIdx.x;
            const uint32_t units = wpb * (KID_TAPER * half + (G - half));
            const uint32_t unit = (nb2 + units - 1u) / units;
            const uint32_t mine = wg < half ? KID_TAPER : 1u;
            const uint64_t ufirst = (uint64_t)wpb * (wg < half ? KID_TAPER * wg : KID_TAPER * half + (wg - half)) + (uint64_t)wib * mine;
            const uint64_t f64 = ufirst * unit;
            duo_first = f64 < nb2 ? (uint32_t)f64 : nb2;
            cnt = nb2 - duo_first < mine * unit ? nb2 - duo_first : mine * unit;
            rd_first = duo_first;
            rd_stride = 1u;
            reads_done = cnt;
        }
        // ---- the read text.  A read of the pair kernel (<= 128 k-mers, k <= 31, behind a shift of <= 15 bases) lies
        // in the first 176 bytes from its 16-byte boundary, one of the duo kernel (<= 256 k-mers) in the first 304:
        // lane l loads bytes [BPL l, BPL l + BPL) of them -- BPL = 4 bases per lane (pair) or 8 (duo), one load
        // instruction per read -- and only the lanes whose bytes hold bases of the read ask (exec is narrowed inside the
        // statement: the compiler must not see a load in a branch of its own).  Nothing beyond the dword that holds the
        // read's last classified base is touched, so the caller's buffer needs no padding beyond its own 16 bytes.
        constexpr uint32_t BPL = PAIRK == 1 ? 4u : 8u;
        typedef typename std::conditional<PAIRK == 1, uint32_t, kid_u2>::type Raw;
        const uint32_t lane_off = lane * BPL;
        auto ask_lanes = [&](const uint32_t sh, const uint32_t nk) -> uint64_t { // the lanes that hold bases of a read (never none: a load always goes out)
            const uint32_t nl = nk ? (sh + nk + (uint32_t)k - 1u + BPL - 1u) / BPL : 1u; // <= 44 (pair), 38 (duo)
            return (1ull << nl) - 1ull;
        };
        // descriptors, 64 at a time: lane l holds the one of read number blk + l of this wave -- the low word
        // of first_base, and its high word (< 2^16: a batch is smaller than 2^48 bytes) with n_kmers (<= 256
        // in these kernels) above it.  Fixed layout: worked out on the spot, there are no descriptors in memory.
        uint32_t blk = 0, dv_lo = 0, dv_hn = 0;
        auto load_descs = [&](const uint32_t first, const uint32_t len) { // reads first .. first + len - 1 of the launch -> lanes 0 .. len - 1
            KidReadDesc d;
            d.first_base = 0; d.n_kmers = 0; d.pad = 0;
            const uint32_t rr = first + lane;
            const KidReadDesc *const dp = static_cast<const KidReadDesc *>(rare->desc);
            if (lane < len) {
                if (dp) d = dp[rr];
                else { d.first_base = (rare->read0 + rr) * (unsigned long long)rare->fixed_len; d.n_kmers = rare->fixed_nk; }
            }
            dv_lo = (uint32_t)d.first_base;
            dv_hn = ((uint32_t)(d.first_base >> 32) & 0xFFFFu) | ((d.n_kmers > 0 ? (uint32_t)d.n_kmers : 0u) << 16);
            if (PAIRK == 1 && lane < len) RG[(blk + lane) & 127u] = rr;
        };
        auto issue_words = [&](const uint32_t idx, Raw &x) {
            const uint32_t hn = (uint32_t)__builtin_amdgcn_readlane((int)dv_hn, (int)idx); // [15:0] first_base >> 32, [30:16] n_kmers
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)dv_lo, (int)idx);
            const uint64_t w0 = (((uint64_t)(hn & 0xFFFFu) << 32) | lo) >> 4;
            // (said once more that this is wave-uniform: under register pressure hipcc has moved such address arithmetic
            //  to the vector ALU and then handed the "s" operand below a VGPR pair -- a build error, seen once)
            const uint8_t *const p = reinterpret_cast<const uint8_t *>(uniform64((uint64_t)(b.bases + 16ull * w0)));
            const uint64_t lanes = ask_lanes(lo & 15u, (hn >> 16) & 0x7FFFu);
            uint64_t save;
            if constexpr (PAIRK == 1)
                asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, %4\n\tglobal_load_dword %0, %2, %3\n\ts_mov_b64 exec, %1"
                             : "+v"(x), "=&s"(save) : "v"(lane_off), "s"(p), "s"(lanes) : "memory");
            else
                asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, %4\n\tglobal_load_dwordx2 %0, %2, %3\n\ts_mov_b64 exec, %1"
                             : "+v"(x), "=&s"(save) : "v"(lane_off), "s"(p), "s"(lanes) : "memory");
        };
        // ASCII -> packed words, in registers.  A lane packs its own 4 (8) bases (kid_codes4), shifts them to their place
        // in the read's 16-base word, and the 4 (2) lanes of a word OR their parts together over DPP quad permutes:
        // afterwards every lane of the group holds the whole word, which is where group_front's ds_bpermute looks for
        // it.  Returns "no base of the read resets a window": decided on the scalar unit from the ballot of the lanes
        // whose bytes hold something that is not ACGT -- the lanes that did not ask hold stale text, and the first and
        // the last lane of a read also hold bytes in front of / behind it (the neighbouring read; the line ends of a
        // FASTQ block), which must not count.  Only for a read that does have such a base are the 16-bit masks of its
        // words put together (wi; else 0: nobody looks).
        const uint32_t part_c = PAIRK == 1 ? 24u - 8u * (lane & 3u) : 16u - 16u * (lane & 1u); // where a lane's codes go in its word
        auto pack_lanes = [&](const Raw x, const uint32_t sh, const uint32_t nk, uint32_t &wc, uint32_t &wi) -> bool {
            uint32_t c, d0, d1 = 0;
            if constexpr (PAIRK == 1) c = kid_codes4(x, db.u_is_t, d0);
            else c = (kid_codes4(x.x, db.u_is_t, d0) << 8) | kid_codes4(x.y, db.u_is_t, d1);
            c <<= part_c;
            c |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0xB1, 0xF, 0xF, false);   // quad_perm:[1,0,3,2]
            if constexpr (PAIRK == 1) c |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x4E, 0xF, 0xF, false); // quad_perm:[2,3,0,1]
            wc = c;
            wi = 0;
            const uint64_t bad = __ballot((d0 | d1) != 0) & ask_lanes(sh, nk);
            if (bad == 0 || nk == 0) return true;
            // (rare, wave-uniform from here on) bytes [sh, end) of the loaded text are the read's
            const uint32_t end = sh + nk + (uint32_t)k - 1u, lf = sh / BPL, ll = (end - 1u) / BPL;
            uint64_t inside = bad & ~((1ull << lf) | (1ull << ll));
            if (inside == 0) { // only the two lanes at the read's ends: look at their bytes
                auto lane_bytes = [&](const uint32_t l) -> uint64_t {
                    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)d1, (int)l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)d0, (int)l);
                };
                const uint64_t all = BPL == 4u ? 0xFFFFFFFFull : ~0ull;
                const uint64_t from = all << (8u * (sh % BPL)), upto = all >> (8u * (BPL - 1u - ((end - 1u) % BPL)));
                inside = lf == ll ? (lane_bytes(lf) & from & upto) : ((lane_bytes(lf) & from) | (lane_bytes(ll) & upto));
            }
            if (inside == 0) return true;
            uint32_t iv = PAIRK == 1 ? kid_inv4(d0) << (4u * (lane & 3u)) : (kid_inv4(d0) | (kid_inv4(d1) << 4)) << (8u * (lane & 1u));
            iv |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)iv, 0xB1, 0xF, 0xF, false);
            if constexpr (PAIRK == 1) iv |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)iv, 0x4E, 0xF, 0xF, false);
            wi = iv;
            return false;
        };
        typedef typename std::conditional<DIGEST, kid_u2, kid_u4>::type Hdr; // what a lookup's first load brings
        auto issue_header = [&](const Group &g, const int u) -> Hdr {
            Hdr v;
            if constexpr (DIGEST) {
                const uint2 *const p = db.digest + (g.act[u] ? g.hlo[u] : 0u);
                asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(v) : "v"(p) : "memory");
            } else {
                const uint4 *const p = db.table + (g.act[u] ? g.hlo[u] * KID_LINE_CELLS : 0u);
                asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(p) : "memory");
            }
            return v;
        };
        auto landed = [](const Hdr &v) { // the loaded registers as the group keeps them
            if constexpr (DIGEST) return make_uint2(v.x, v.y);
            else return make_uint4(v.x, v.y, v.z, v.w);
        };
        Raw xA{}, xB{};
        if constexpr (PAIRK == 2) {
            load_descs(duo_first, cnt < 64u ? cnt : 64u);
            issue_words(0u, xA);
            issue_words(1u, xB);
            // ---- reads of two groups (129..256 k-mers: 2 x 250 bp): the pair is the two groups of ONE read.
            // They share the read's words, their queue entries carry the same tag, and the read stays open in the
            // resolver between them.  Two text registers alternate, each requested two trips ahead (a trip is one
            // read here).
            auto duo = [&](const uint32_t i, Raw &xC) { // xC: the register that holds the text of read i
                const uint32_t ia = i - blk;
                const uint32_t hnC = (uint32_t)__builtin_amdgcn_readlane((int)dv_hn, (int)ia);
                const uint32_t nk = (hnC >> 16) & 0x7FFFu;
                const uint32_t sh = (uint32_t)__builtin_amdgcn_readlane((int)dv_lo, (int)ia) & 15u;
                const uint32_t nb = nk + (uint32_t)k - 1;
                Group gA, gB;
                uint32_t bad = 0;
                if (ia + 2u > 63u) { // (this read's descriptor is in scalars by now)
                    blk = i + 1u;
                    load_descs(duo_first + blk, cnt - blk < 64u ? cnt - blk : 64u);
                }
                asm volatile("s_waitcnt vmcnt(1)" : "+v"(xC) : : "memory"); // behind: the text of the next read (other register)
                uint32_t cC, iC;
                const bool cl = pack_lanes(xC, sh, nk, cC, iC);
                group_front(nullptr, sh, nb, nk, 0u, cl, gA, bad, false, cC, iC);
                Hdr hA0 = issue_header(gA, 0), hA1 = issue_header(gA, 1);
                group_front(nullptr, sh, nb, nk, (uint32_t)(U * 64), cl, gB, bad, false, cC, iC);
                Hdr hB0 = issue_header(gB, 0), hB1 = issue_header(gB, 1);
                issue_words(i + 2u - blk, xC); // this register is used up: the read after the next, two trips ahead
                n_lookups += nk - bad;
                asm volatile("s_waitcnt vmcnt(3)" : "+v"(hA0), "+v"(hA1) : : "memory"); // behind: the headers of B, the text just requested
                gA.hd[0] = landed(hA0);
                gA.hd[1] = landed(hA1);
                bool had = back_deferred(gA, i);
                if (qn >= KID_CQ_FLUSH) resolve_all(i, i & 63u); // the read stays open
                asm volatile("s_waitcnt vmcnt(1)" : "+v"(hB0), "+v"(hB1) : : "memory"); // behind: the text just requested
                gB.hd[0] = landed(hB0);
                gB.hd[1] = landed(hB1);
                had |= back_deferred(gB, i);
                if (!had) commit_zero(i);
                else if (qn >= KID_CQ_FLUSH) resolve_all(i, 0xFFFFFFFFu);
                if (((i + 1u) & 63u) == 0u) { // tags and result slots are read numbers mod 64
                    if (qn || cur_tag != 0xFFFFFFFFu) resolve_all(i, 0xFFFFFFFFu);
                    flush_results(i + 1u - 64u, 64u);
                }
            };
            for (uint32_t i = 0; i < cnt; i += 2) {
                duo(i, xA);
                if (i + 1u < cnt) duo(i + 1u, xB);
            }
            if (qn || cur_tag != 0xFFFFFFFFu) resolve_all(cnt - 1u, 0xFFFFFFFFu);
            if (cnt & 63u) flush_results(cnt & ~63u, cnt & 63u);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(xA), "+v"(xB) : : "memory");
        } else {
        // ---- the pair kernel.  A wave takes blocks of 64 CONSECUTIVE reads: the text (9.6 KB at 150 bp) and the results
        // (256 bytes) of a block are lines that no other wave -- no other L2 -- touches; its blocks are one contiguous
        // share of the launch.  Shares shrink: the first half of the workgroups (dispatched first) take KID_TAPER units
        // of reads per wave, the second half one.  Workgroups take 200-330 us for the same number of reads (the SIMDs
        // serve their oldest waves first), and a launch ends when the slowest of its last workgroups does: with equal
        // shares the chip idles through half the spread of a 250-us workgroup at the end of a 1-ms launch, with small
        // last shares through a third of that (profiles/r02/ab_taper.txt, ab_block_cyclic.txt).
        const uint32_t n32 = (uint32_t)b.n;
        uint32_t seq = 0;        // wave-local number of the pair's first read (even)
        uint32_t blen = 0;       // reads in the current block [blk, blk + blen)
        uint32_t nreal = 0;      // reads classified
        uint32_t sblk = 0;       // number of the wave's next block
        // the next block (length 0: none) and its descriptors: lane l holds the one of wave-local read blk + l
        auto switch_block = [&]() {
            const uint32_t G = gridDim.x, half = G >> 1, wg = blockIdx.x;
            const uint32_t units = wpb * (KID_TAPER * half + (G - half));    // shares of one unit per wave
            const uint32_t unit = (((n32 + units - 1u) / units) + 1u) & ~1u; // reads per unit (even)
            const uint32_t mine = wg < half ? KID_TAPER : 1u;
            const uint64_t ufirst = (uint64_t)wpb * (wg < half ? KID_TAPER * wg : KID_TAPER * half + (wg - half)) + (uint64_t)wib * mine;
            const uint64_t wave_first = ufirst * unit, off = (uint64_t)sblk * 64u, wave_cnt = (uint64_t)mine * unit;
            sblk++;
            const uint64_t f64 = wave_first + off;
            const uint32_t first = f64 < n32 ? (uint32_t)f64 : n32;
            uint32_t len = off < wave_cnt ? (uint32_t)(wave_cnt - off < 64u ? wave_cnt - off : 64u) : 0u;
            if (len > n32 - first) len = n32 - first;
            load_descs(first, len);
            blen = len;
        };
        switch_block();
        bool more = blen != 0;
        if (more) {
            issue_words(0u, xA);
            issue_words(1u, xB);
        }
        while (more) {
            const uint32_t i = seq;
            const uint32_t ia = i - blk;
            const uint32_t hnA = (uint32_t)__builtin_amdgcn_readlane((int)dv_hn, (int)ia), hnB = (uint32_t)__builtin_amdgcn_readlane((int)dv_hn, (int)(ia + 1u));
            const uint32_t nkA = (hnA >> 16) & 0x7FFFu, nkB = (hnB >> 16) & 0x7FFFu;
            const uint32_t shA = (uint32_t)__builtin_amdgcn_readlane((int)dv_lo, (int)ia) & 15u;
            const uint32_t shB = (uint32_t)__builtin_amdgcn_readlane((int)dv_lo, (int)(ia + 1u)) & 15u;
            const bool realB = ia + 1u < blen; // (a block with an odd number of reads -- the last of a share: B is a phantom of zero k-mers)
            Group gA, gB;
            uint32_t badA = 0, badB = 0;
            // the block's last pair: the next block's descriptors (this pair's are in scalars by now)
            if (ia + 2u >= blen) {
                blk = i + 2u;
                switch_block(); // (no block: all-zero descriptors, the requests below fetch four bytes nobody needs)
                more = blen != 0;
            }

            // The text of the next pair is requested as soon as this pair's is used up, a whole trip ahead:
            // it comes from HBM (a batch is larger than the L2).
            asm volatile("s_waitcnt vmcnt(1)" : "+v"(xA) : : "memory"); // behind: the text of B
            uint32_t cA, iA;
            const bool clA = pack_lanes(xA, shA, nkA, cA, iA); // no base of the read resets a window
            group_front(nullptr, shA, nkA + (uint32_t)k - 1, nkA, 0u, clA, gA, badA, false, cA, iA);
            Hdr hA0 = issue_header(gA, 0), hA1 = issue_header(gA, 1);
            issue_words(i + 2u - blk, xA);

            asm volatile("s_waitcnt vmcnt(3)" : "+v"(xB) : : "memory"); // behind: headers of A, next text of A
            uint32_t cB, iB;
            const bool clB = pack_lanes(xB, shB, nkB, cB, iB);
            group_front(nullptr, shB, nkB + (uint32_t)k - 1, nkB, 0u, clB, gB, badB, false, cB, iB);
            Hdr hB0 = issue_header(gB, 0), hB1 = issue_header(gB, 1);
            issue_words(i + 3u - blk, xB);

            asm volatile("s_waitcnt vmcnt(4)" : "+v"(hA0), "+v"(hA1) : : "memory"); // behind: next text of A, headers and next text of B
            gA.hd[0] = landed(hA0);
            gA.hd[1] = landed(hA1);
            n_lookups += nkA - badA;
            if (!back_deferred(gA, i)) commit_zero(i);
            else if (qn >= KID_CQ_FLUSH) resolve_all(i, 0xFFFFFFFFu);

            asm volatile("s_waitcnt vmcnt(1)" : "+v"(hB0), "+v"(hB1) : : "memory"); // behind: the next text of B
            gB.hd[0] = landed(hB0);
            gB.hd[1] = landed(hB1);
            nreal += realB ? 2u : 1u;
            if (realB) {
                n_lookups += nkB - badB;
                if (!back_deferred(gB, i + 1u)) commit_zero(i + 1u);
                else if (qn >= KID_CQ_FLUSH) resolve_all(i + 1u, 0xFFFFFFFFu);
            }
            seq = i + 2u;
            if ((seq & 63u) == 0u) { // tags and result slots are wave-local read numbers mod 64
                if (qn) resolve_all(i + 1u, 0xFFFFFFFFu);
                flush_results(seq - 64u, 64u);
            }
        }
        // (the two requests behind the last pair fetched text nobody needs)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xA), "+v"(xB) : : "memory");
        // a block of odd length ends the wave's work: seq counts its phantom, the flush below must not
        if (nreal & 1u) seq -= 1u;
        reads_done = seq;
        if (qn) resolve_all(seq - 1u, 0xFFFFFFFFu);
        if (seq & 63u) flush_results(seq & ~63u, seq & 63u);
        }
    }
    if constexpr (PAIRK == 0) {
        // Software pipeline, unrolled by two with two named register sets (A, B) so that nothing is
        // copied between stages: the descriptor of a read is requested two reads ahead (scalar loads)
        // and its first packed words one read ahead; the waits the compiler places in front of their
        // first use land behind a whole read's worth of work.  32-bit read indices (n < 2^31).
        const uint32_t n32 = (uint32_t)b.n;
        // the wave's reads: rd_first + i rd_stride, i < gen_cnt -- a strided share of the batch, or (KID_TAPER, minimizer-
        // localised table) one contiguous range in the pair kernel's shrinking shares
        gen_cnt = gw32 < n32 ? (n32 - gw32 + nw32 - 1u) / nw32 : 0u;
        if (MINLOC) {
            const uint32_t G = gridDim.x, half = G >> 1, wg = blockIdx.x;
            const uint32_t units = wpb * (KID_TAPER * half + (G - half));
            const uint32_t unit = (n32 + units - 1u) / units;
            const uint32_t mine = wg < half ? KID_TAPER : 1u;
            const uint64_t ufirst = (uint64_t)wpb * (wg < half ? KID_TAPER * wg : KID_TAPER * half + (wg - half)) + (uint64_t)wib * mine;
            const uint64_t f64 = ufirst * unit;
            rd_first = f64 < n32 ? (uint32_t)f64 : n32;
            rd_stride = 1u;
            gen_cnt = n32 - rd_first < mine * unit ? n32 - rd_first : mine * unit;
            reads_done = gen_cnt;
        }
        const uint32_t gf = rd_first, gs = rd_stride, gc = gen_cnt;
        KidReadDesc dA, dB;
        kid_u4 xA, xB;
        fetch_desc(gc > 0u ? gf : n32, dA);
        fetch_desc(gc > 1u ? gf + gs : n32, dB);
        fetch_words(dA, xA);
        for (uint32_t i = 0; i < gc; i += 2) { // i: number of the read within this wave
            const uint32_t r = gf + i * gs;
            short_read(r, i, uniform64(dA.first_base), __builtin_amdgcn_readfirstlane(dA.n_kmers), xA,
                       [&]() { fetch_words(dB, xB); fetch_desc(i + 2u < gc ? r + 2u * gs : n32, dA); });
            if (i + 1u >= gc) break;
            short_read(r + gs, i + 1u, uniform64(dB.first_base), __builtin_amdgcn_readfirstlane(dB.n_kmers), xB,
                       [&]() { fetch_words(dA, xA); fetch_desc(i + 3u < gc ? r + 3u * gs : n32, dB); });
            if (MINLOC && ((i + 2u) & 63u) == 0u) { // tags and result slots are read numbers mod 64
                if (qn || cur_tag != 0xFFFFFFFFu) resolve_all(i + 1u, 0xFFFFFFFFu);
                flush_results(i + 2u - 64u, 64u);
            }
        }
        if (MINLOC) {
            const uint32_t cnt = gc;
            if (qn || cur_tag != 0xFFFFFFFFu) resolve_all(cnt - 1u, 0xFFFFFFFFu);
            if (cnt & 63u) flush_results(cnt & ~63u, cnt & 63u);
        }
    }
    // ---- phase 2: the long reads this wave met (FASTA records, long-read data), one at a time
    if (PAIRK == 0 && any_long) {
        rb_direct = true; // the other reads' results are stored already: these go out one by one
        for (uint32_t i = 0; i < gen_cnt; i++) {
            const uint64_t r = (uint64_t)rd_first + (uint64_t)i * rd_stride;
            KidReadDesc d;
            fetch_desc((uint32_t)r, d);
            const int64_t nk = (int64_t)__builtin_amdgcn_readfirstlane(d.n_kmers);
            if (nk <= KID_SEG_KMERS) continue;
            kid_u4 x0;
            fetch_words(d, x0);
            process_read(r, i, uniform64(d.first_base), nk, x0, []() {});
            if (MINLOC && (qn || cur_tag != 0xFFFFFFFFu)) resolve_all(i, 0xFFFFFFFFu);
        }
    }
    if (MINLOC && lane == 0) atomicAdd(WL, (unsigned long long)n_lookups);
    if (MINLOC && n_zero && lane == 0) {
        if (HIST) atomicAdd(&hist[0], n_zero); // low half = target 0; a workgroup stays below 65536 reads
        else atomicAdd(&rare->gcount[0], (unsigned long long)n_zero);
    }
    if (!HIST && pend_n && lane == 0) atomicAdd(&rare->gcount[pend_t], (unsigned long long)pend_n);

    // ---- flush (with the minimizer-localised table the histogram packs two 16-bit counters per word:
    // the host keeps a workgroup below 65536 reads per launch)
    if (HIST) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < hist_words; i += blockDim.x) {
            const uint32_t v = hist[i];
            if (MINLOC) {
                if (v & 0xFFFFu) atomicAdd(&rare->gcount[2u * i], (unsigned long long)(v & 0xFFFFu));
                if (v >> 16) atomicAdd(&rare->gcount[2u * i + 1u], (unsigned long long)(v >> 16));
            } else if (v) atomicAdd(&rare->gcount[i], (unsigned long long)v);
        }
    }
    if (lane == 0) {
        const unsigned long long tl = *WL, n_reads = reads_done;
        const uint32_t n_hits = WC[2];
        const unsigned long long te = WC[3];
        if (n_reads) atomicAdd(&WGS[0], n_reads);
        if (tl) atomicAdd(&WGS[1], tl);
        if (tl + te) atomicAdd(&WGS[2], tl + te); // cells read: one per lookup plus the probes beyond the first
        if (n_hits) atomicAdd(&WGS[3], (unsigned long long)n_hits);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = WGS[threadIdx.x];
        if (v) atomicAdd(&rare->stats[threadIdx.x], v);
    }
    if (threadIdx.x == 0) {
        // The launch's last workgroup banks the interval ([6] += ticks, [7] += 1) and re-arms the stamps for the next
        // launch.  Everything here is an atomic performed in memory, one after the other (each returns before the next is
        // issued): no fence -- a release / acquire fence at device scope writes back and invalidates the L2 of the
        // wave's XCD (buffer_wbl2 / buffer_inv sc1), and 4096 of those per launch cost 0.2 ms of 1.1
        // (profiles/r03/bench_fence_in_epilogue.json).
        unsigned long long prev = atomicMax(&s.stats[31], (unsigned long long)__builtin_amdgcn_s_memrealtime());
        asm volatile("" : "+v"(prev)); // (the stamp is in memory before this workgroup counts itself out)
        unsigned long long done = atomicAdd(&s.stats[29], 1ull);
        if (done + 1ull == (unsigned long long)gridDim.x) {
            const unsigned long long a = atomicAdd(&s.stats[30], 0ull), z = atomicAdd(&s.stats[31], 0ull);
            if (z > a) { atomicAdd(&s.stats[6], z - a); atomicAdd(&s.stats[7], 1ull); }
            unsigned long long t0 = atomicExch(&s.stats[30], ~0ull), t1 = atomicExch(&s.stats[31], 0ull);
            asm volatile("" : "+v"(t0), "+v"(t1));
            atomicExch(&s.stats[29], 0ull);
        }
    }
}

#include "kid_probes.hip.h"
#include "kid_insert.hip.h"
