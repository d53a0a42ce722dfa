// kid_table.hip.h -- what every kernel knows of the database and a batch: the device structs, the cell loads, the
// lookup in both table geometries, the DPP row scans of the sliding minimum and msca on rows or by climbing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "kid_common.h"

#define KID_WAVE 64
#define KID_TOMBSTONE_HI 0xFFFFFFFFu // high key word of a duplicate entry that lost to an earlier insert (keys are < 2^62)

typedef uint32_t kid_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t kid_u2 __attribute__((ext_vector_type(2)));

// One table cell.  Reference placement: non-temporal -- a probe touches a random 16 bytes of a 16 GiB
// table once, so the line is not worth keeping in L2 / Infinity Cache (tools/gather_policy.hip: 49 ->
// 54 G random cells/s on a 16 GiB region).  Minimizer-localised placement: plain loads -- the header
// of a line is read again by the resolver and the matching entry sits in the same 128 bytes, so the
// line should stay cached (measured: 1.29 -> 1.23 ms per launch).
// Fire-and-forget global writes of the classify kernel (per-read result, seen-bitmap bits).  Issued
// from inline assembly so that the compiler's waitcnt insertion does not know them: on gfx9 a pending
// store or no-return atomic shares vmcnt with the loads and makes the next wait a full vmcnt(0) drain,
// i.e. every read would sit out the write acknowledgement of the one before.  Nothing in the kernel
// reads these locations back; they complete before the kernel does.
__device__ __forceinline__ void kid_store_u32_nowait(uint32_t *p, uint32_t v)
{
    asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void kid_atomic_or_nowait(uint32_t *p, uint32_t v)
{
    asm volatile("global_atomic_or %0, %1, off" : : "v"(p), "v"(v) : "memory");
}

__device__ __forceinline__ uint4 kid_load_cell(const uint4 *table, uint32_t idx) { return table[idx]; }
__device__ __forceinline__ uint4 kid_load_cell_nt(const uint4 *table, uint32_t idx)
{
    const kid_u4 v = __builtin_nontemporal_load(reinterpret_cast<const kid_u4 *>(table) + idx);
    return make_uint4(v.x, v.y, v.z, v.w);
}

struct KidDevDb {
    const uint4 *table;
    uint64_t nslots;
    uint32_t slot_mask;
    uint32_t max_probes;
    int k;
    uint32_t u_is_t;
    uint32_t minloc; // 1: minimizer-localised geometry (kid_common.h), 0: the reference's fmix64 + triangular probing
    uint32_t line_shift; // minloc: 32 - log2(lines)
    uint32_t line_mask;  // minloc: lines - 1
    const uint4 *rows; // null when the tree does not fit the row encoding
    const int32_t *parent;
    const int32_t *depth;
    int32_t ntar;
    const uint2 *digest; // minloc, GPU-built: the digest plane, 8 bytes per line (kid_common.h); null: the table has none
};

struct KidBatch { // what the caller handed over
    const uint8_t *bases;
    const uint64_t *offsets; // null: fixed_len layout
    const int32_t *start;    // nullable
    const int32_t *stop;     // nullable
    uint32_t *out_final;     // nullable
    uint64_t n;
    uint32_t fixed_len;
};

// per-read descriptor written by kid_prepare_kernel: absolute index of the first base of the
// classified range and the number of k-mer windows in it (<= 0: none)
struct KidReadDesc {
    uint64_t first_base;
    int32_t n_kmers;
    uint32_t pad;
};

// Very long records (FASTA contigs classified whole, kmer_read_vf6.cpp:803-861).  The classify kernels give a read to ONE
// wave; a record of more than `long_cut` k-mers goes to the long-record kernels instead (kid_long_*): kid_prepare_kernel
// hides it from the classify kernels (n_kmers = 0) and puts it on this list, kid_long_plan_kernel turns the list into
// the records' places in the hit array.  All on the device: the batch may be one whose offsets the host never saw.
#define KID_LONG_MAX 1024u
struct KidLongList {
    uint32_t n;       // records flagged so far (beyond KID_LONG_MAX: left to the classify kernels)
    uint32_t pad[3];
    struct Item { uint64_t first_base; uint32_t n_kmers; uint32_t read; } e[KID_LONG_MAX];
};
struct KidLongRec {
    uint64_t first_base; // absolute index of the record's first classified base in the batch text
    uint64_t hits_off;   // where its hits start in the hits array
    uint32_t n_kmers;
    uint32_t read;       // its number in the batch
    uint64_t tile0;      // number of 256-position tiles of the records before it
};
struct KidLongPlan {
    uint32_t n_recs;
    uint32_t pad;
    uint64_t n_tiles;
    uint64_t total_kmers;
    KidLongRec recs[KID_LONG_MAX];
};

// What a launch of the classify kernels reads: the ASCII read text as the caller handed it over -- the kernels turn it
// into 2-bit codes in registers (kid_pack4 / kid_pack16), there is no packed image of the batch in memory -- and the
// reads' descriptors.  Fixed layout (kid_classify_fixed_*): no descriptors either, read r of the launch is
// bases[(read0 + r) * fixed_len ...) with fixed_nk k-mers (KidRareArgs).
struct KidInput {
    const uint8_t *bases;    // 16-byte aligned; readable up to 16 bytes past the last read
    const KidReadDesc *desc; // of this launch's reads; null: fixed layout
    uint32_t *out_final;     // of this launch's reads; nullable
    uint64_t n;              // reads of this launch
};

struct KidSampleDev {
    unsigned long long *gcount;
    uint32_t *seen;
    unsigned long long *stats; // [0] reads [1] lookups [2] probes [3] hits [4] argument errors [5] FASTQ records dropped by process_qual
                               // [6] device-clock ticks [7] launches banked [8] quality lines shorter than their sequence
                               // [29] workgroups through [30] first start [31] last end of the running launch
};

// What only rare paths of the classify kernel need (hit cells, the flush at the end): kept in device
// memory and loaded where used, so it does not occupy scalar registers across the hot loop.
struct KidRareArgs {
    unsigned long long *gcount;
    unsigned long long *stats;
    uint32_t line_mask;
    uint32_t fixed_len;           // fixed layout: bases per read (0: the launch has descriptors)
    unsigned long long batch_max; // (batch sequence number << 32) | largest n_kmers of the batch: kid_prepare_kernel
    unsigned long long read0;     // fixed layout: number of the launch's first read within the batch text
    int32_t fixed_nk;             // fixed layout: k-mers per read
    uint32_t pad;
    // what the resolver / the 64-read flush of the pair kernels need (rare paths by now, bulk work: a scalar
    // load there is cheaper than four scalar registers held across the hot loop)
    const uint4 *rows;
    uint32_t *seen;
    uint32_t *out_final;   // of the current launch: written by kid_prepare_kernel / kid_rebase_kernel
    const void *desc;      // of the current launch (KidReadDesc *; null: fixed layout)
    // the hit log (see kid_seenlog_*): the resolver appends the entry ordinals of its hits instead of setting their bits
    // in `seen` with one memory-side atomic each; null: atomics
    uint32_t *seen_log;      // KID_LOG_SHARDS regions of seen_log_cap entries
    uint32_t *seen_log_tail; // their fill counters, 64 bytes apart
    uint32_t seen_log_cap;
    uint32_t pad2;
    const uint4 *table;      // the DIGEST instantiations keep the plane's pointer in scalar registers, not the table's
};

// ------------------------------------------------------------------ hash lookup
// Hashtable::getHash, newkmer_10nx.cpp:204-233 (+ probe cap kmer_read_m3.cpp:232)
// Candidate entries of a line header for fingerprint fp, as a bit set: bit (15 - d) = entry 2d,
// bit (31 - d) = entry 2d + 1 (d = header dword 0..3).  A superset of the true matches (the classic
// zero-halfword test can also flag the upper half of a dword whose lower half matched); every
// candidate is verified against the full key, so a false one only costs a load.
__device__ __forceinline__ uint32_t kid_hdr_cand(const uint4 &h, uint32_t fp)
{
    const uint32_t rep = fp * 0x00010001u, one = 0x00010001u, top = 0x80008000u;
    const uint32_t a = h.x ^ rep, b = h.y ^ rep, c = h.z ^ rep, d = (h.w ^ rep) | 0xFFFF0000u; // upper half of .w = count
    return (((a - one) & ~a) & top) | ((((b - one) & ~b) & top) >> 1) | ((((c - one) & ~c) & top) >> 2) |
           ((((d - one) & ~d) & top) >> 3);
}
// the same question as a yes/no, written as seven 16-bit compares: hipcc turns them into
// v_cmp_eq_u16 with sub-dword operand selects, whose lane masks combine on the scalar unit
__device__ __forceinline__ bool kid_hdr_any(const uint4 &h, uint32_t fp)
{
    const uint16_t f = (uint16_t)fp;
    return ((uint16_t)h.x == f) | ((uint16_t)(h.x >> 16) == f) | ((uint16_t)h.y == f) | ((uint16_t)(h.y >> 16) == f) |
           ((uint16_t)h.z == f) | ((uint16_t)(h.z >> 16) == f) | ((uint16_t)h.w == f);
}
__device__ __forceinline__ uint32_t kid_cand_entry(uint32_t bit) // bit index from kid_hdr_cand -> entry 0..6
{
    return 2u * (15u - (bit & 15u)) + (bit >> 4);
}

// Lookup in the minimizer-localised table: header, then the candidate entries, then the next line
// while the chain continues.  Returns the target (0 = absent); ncell = cells read.
__device__ __forceinline__ uint32_t kid_bucket_lookup(const KidDevDb &db, uint64_t key, uint32_t g, uint32_t &slot, uint32_t &ncell)
{
    uint32_t line = kid_minloc_line(g, db.line_shift);
    const uint32_t fp = kid_key_fp(key);
    ncell = 0;
    slot = 0;
    for (;;) {
        const uint32_t base = line * KID_LINE_CELLS;
        const uint4 h = db.table[base];
        ncell++;
        uint32_t m = kid_hdr_cand(h, fp);
        while (m) {
            const uint32_t j = kid_cand_entry((uint32_t)__builtin_ctz(m));
            m &= m - 1;
            const uint4 c = db.table[base + 1u + j];
            ncell++;
            if (c.z != 0 && c.x == (uint32_t)key && c.y == (uint32_t)(key >> 32)) { slot = c.w - 1u; return c.z; }
        }
        if (!kid_hdr_continues(h.w, fp)) return 0;
        line = (line + 1u) & db.line_mask;
    }
}

__device__ __forceinline__ uint32_t kid_dev_lookup(const KidDevDb &db, uint64_t key, uint32_t &slot, uint32_t &nprobe)
{
    uint32_t i = 0, res = 0;
    slot = 0;
    if (db.minloc) return kid_bucket_lookup(db, key, kid_minimizer_of_key(key, db.k), slot, nprobe);
    const uint64_t hash = kid_fmix64(key);
    uint64_t reprobe = 0;
    do {
        const uint32_t idx = ((uint32_t)hash + (uint32_t)reprobe) & db.slot_mask;
        reprobe += ++i;
        const uint4 c = db.table[idx];
        if (c.z == 0) break;
        if (c.x == (uint32_t)key && c.y == (uint32_t)(key >> 32)) { res = c.z; slot = c.w - 1u; break; }
    } while (reprobe < db.nslots && (db.max_probes == 0 || i < db.max_probes));
    nprobe = i;
    return res;
}

// ------------------------------------------------------------------ sliding-window minimum over a wavefront
// 16-lane DPP rows double as the blocks of the van Herk / Gil-Werman scheme: with P = prefix
// minimum and S = suffix minimum inside each row, min(a[p..p+15]) = min(S[p], P[p+15]).
// (a lane whose DPP source lies outside its row is disabled for that instruction: it keeps its own value.  A VGPR written
//  by a VALU instruction may be read through DPP two wait states later: s_nop 1 between dependent steps of ONE scan;
//  kid_row_scans interleaves four scans instead)
__device__ __forceinline__ uint32_t kid_row_prefix_min(uint32_t x)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x111, 0xF, 0xF, false); x = x < t ? x : t; // row_shr:1
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x112, 0xF, 0xF, false); x = x < t ? x : t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x114, 0xF, 0xF, false); x = x < t ? x : t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x118, 0xF, 0xF, false); x = x < t ? x : t;
    return x;
}
__device__ __forceinline__ uint32_t kid_row_suffix_min(uint32_t x)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x101, 0xF, 0xF, false); x = x < t ? x : t; // row_shl:1
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x102, 0xF, 0xF, false); x = x < t ? x : t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x104, 0xF, 0xF, false); x = x < t ? x : t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)x, 0x108, 0xF, 0xF, false); x = x < t ? x : t;
    return x;
}
// prefix and suffix minima of two tiles at once: p0 = s0 = hashes of the first tile, p1 = s1 = those of the second
__device__ __forceinline__ void kid_row_scans(uint32_t &p0, uint32_t &s0, uint32_t &p1, uint32_t &s1)
{
    p0 = kid_row_prefix_min(p0); s0 = kid_row_suffix_min(s0);
    p1 = kid_row_prefix_min(p1); s1 = kid_row_suffix_min(s1);
}

// ------------------------------------------------------------------ taxonomy
// Tree1::msca, newkmer_10nx.cpp:118-144, on the ancestor-row encoding.
// Let L = deepest common node of the two root paths.  The reference returns x
// when y lies on x's root path (L == y), y when x lies on y's (L == x), else L.
__device__ __forceinline__ uint32_t kid_row_entry(const uint4 &r, uint32_t d)
{
    const uint32_t w = d < 2 ? r.x : d < 4 ? r.y : d < 6 ? r.z : r.w;
    return (d & 1) ? (w >> 16) : (w & 0xFFFFu);
}

__device__ __forceinline__ uint32_t kid_msca_rows(uint32_t x, const uint4 &rx, uint32_t y, const uint4 &ry, uint4 &rout)
{
    const uint32_t dx = rx.x & 0xFFFFu, dy = ry.x & 0xFFFFu;
    const uint64_t lo = ((uint64_t)(rx.y ^ ry.y) << 32) | ((rx.x ^ ry.x) & 0xFFFF0000u);
    const uint64_t hi = ((uint64_t)(rx.w ^ ry.w) << 32) | (rx.z ^ ry.z);
    uint32_t f = lo ? (uint32_t)(__builtin_ctzll(lo) >> 4) : hi ? 4u + (uint32_t)(__builtin_ctzll(hi) >> 4) : 8u;
    uint32_t c = f - 1; // entries 1..f-1 agree
    c = c < dx ? c : dx;
    c = c < dy ? c : dy;
    if (c == 7 && dx == 8 && dy == 8 && x == y) c = 8; // depth-8 nodes are not stored in their own row
    if (c == dy) { rout = rx; return x; }
    if (c == dx) { rout = ry; return y; }
    rout = rx;
    rout.x = (rx.x & 0xFFFF0000u) | c;
    return c == 0 ? 1u : kid_row_entry(rx, c);
}

// An ancestor row on its way between lanes, one function per shape of the move:
// the row lane j holds (j wave-uniform), in every lane
__device__ __forceinline__ uint4 kid_row_of_lane(const uint4 &r, int j)
{
    uint4 o;
    o.x = (uint32_t)__builtin_amdgcn_readlane((int)r.x, j);
    o.y = (uint32_t)__builtin_amdgcn_readlane((int)r.y, j);
    o.z = (uint32_t)__builtin_amdgcn_readlane((int)r.z, j);
    o.w = (uint32_t)__builtin_amdgcn_readlane((int)r.w, j);
    return o;
}
// the row kept in lanes 0-3 of one register, in every lane.  (The way back stays written out where it happens, as
// v = lane == 0 ? r.x : lane == 1 ? r.y : lane == 2 ? r.z : lane == 3 ? r.w : v -- behind a function, by value or by
// reference, hipcc compiles 20 of the classify kernels differently.)
__device__ __forceinline__ uint4 kid_row_unpack(uint32_t v)
{
    uint4 o;
    o.x = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    o.y = (uint32_t)__builtin_amdgcn_readlane((int)v, 1);
    o.z = (uint32_t)__builtin_amdgcn_readlane((int)v, 2);
    o.w = (uint32_t)__builtin_amdgcn_readlane((int)v, 3);
    return o;
}
// the row of the lane each lane names (src = 4 * that lane: a ds_bpermute address)
__device__ __forceinline__ uint4 kid_row_bpermute(int src, const uint4 &r)
{
    uint4 o;
    o.x = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)r.x);
    o.y = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)r.y);
    o.z = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)r.z);
    o.w = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)r.w);
    return o;
}

// same function by climbing parent[]/depth[] (any tree shape)
__device__ __forceinline__ uint32_t kid_msca_climb(const KidDevDb &db, uint32_t x, uint32_t y)
{
    uint32_t a = x, b = y;
    int32_t da = db.depth[a], dd = db.depth[b];
    while (da > dd) { a = (uint32_t)db.parent[a]; da--; }
    while (dd > da) { b = (uint32_t)db.parent[b]; dd--; }
    while (a != b) { a = (uint32_t)db.parent[a]; b = (uint32_t)db.parent[b]; }
    if (a == y) return x;
    if (a == x) return y;
    return a;
}
