// kid_insert.hip.h -- keys and targets -> table cells, in both geometries (kid_build.hip.h makes the keys from genomes).
#pragma once
#include "kid_table.hip.h"

// ------------------------------------------------------------------ table build on the GPU
// Pass 1: every entry claims the first free cell on its probe path (same path
// as Hashtable::add_kmer, newkmer_10nx.cpp:235-263) with a CAS on the ordinal
// word.  Like the reference there is no key comparison: duplicates take
// separate cells.  Entries with target 0 are skipped: in the reference they
// leave their cell "empty" (value == 0), i.e. invisible to every lookup.
// Pass 1: every entry claims a cell.  Reference geometry: the first free cell on the reference's
// probe path (Hashtable::add_kmer, newkmer_10nx.cpp:235-263), claimed with a CAS on the ordinal
// word; like the reference there is no key comparison, duplicates take separate cells.
// Minimizer-localised geometry: the next free entry of the key's line (count in the header,
// CAS), chaining into the following line when 7 entries are taken; the key's 16-bit fingerprint
// goes into the header.  Entries with target 0 are skipped: in the reference they leave their
// cell "empty" (value == 0), i.e. invisible to every lookup.
__global__ void kid_build_insert_kernel(uint4 *table, uint32_t slot_mask, const uint64_t *keys, const uint32_t *targets,
                                        uint64_t n, uint32_t ntar, unsigned long long *n_occupied, int k, uint32_t minloc,
                                        uint32_t line_shift, uint32_t line_mask)
{
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < n; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = targets[e];
        if (t == 0) continue;
        if (t >= ntar) { atomicAdd(n_occupied + 1, 1ull); continue; } // reported as KID_ERR_TARGET
        const uint64_t key = keys[e];
        if (minloc) {
            uint32_t line = kid_minloc_line(kid_minimizer_of_key(key, k), line_shift);
            const uint32_t fp = kid_key_fp(key);
            for (;;) {
                uint32_t *hdr = reinterpret_cast<uint32_t *>(table + (uint64_t)line * KID_LINE_CELLS);
                uint32_t old = __hip_atomic_load(hdr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                uint32_t cnt;
                for (;;) {
                    cnt = kid_hdr_count(old);
                    if (cnt >= KID_HDR_FULL) break;
                    const uint32_t seen = atomicCAS(hdr + 3, old, old + 0x10000u);
                    if (seen == old) break;
                    old = seen;
                }
                if (cnt < KID_LINE_ENTRIES) { // entry number cnt of this line is mine
                    uint32_t *c = reinterpret_cast<uint32_t *>(table + (uint64_t)line * KID_LINE_CELLS + 1u + cnt);
                    c[0] = (uint32_t)key;
                    c[1] = (uint32_t)(key >> 32);
                    c[2] = t;
                    c[3] = (uint32_t)e + 1u;
                    atomicOr(hdr + (cnt >> 1), fp << (16u * (cnt & 1u)));
                    atomicAdd(n_occupied, 1ull);
                    break;
                }
                atomicOr(hdr + 3, 1u << kid_ovf_bit(fp)); // pushed past this line: leave a trace for the lookups
                line = (line + 1u) & line_mask; // cnt == 7 just became 8 (chain marker) or was 8 already
            }
            continue;
        }
        const uint32_t h = (uint32_t)kid_fmix64(key) & slot_mask;
        uint32_t rp = 0, i = 0;
        for (;;) {
            const uint32_t idx = (h + rp) & slot_mask;
            rp += ++i;
            uint32_t *ordp = reinterpret_cast<uint32_t *>(table + idx) + 3;
            if (atomicCAS(ordp, 0u, (uint32_t)e + 1u) == 0u) {
                uint32_t *c = reinterpret_cast<uint32_t *>(table + idx);
                c[0] = (uint32_t)key;
                c[1] = (uint32_t)(key >> 32);
                c[2] = t;
                atomicAdd(n_occupied, 1ull);
                break;
            }
        }
    }
}

// Pass 2: the reference's lookup returns the FIRST-inserted copy of a key (earlier inserts sit
// earlier on the path).  Pass 1 placed duplicate copies in arbitrary order, so every entry walks
// its whole chain, finds the smallest ordinal among the cells holding its key and, unless that is
// its own, turns ITS OWN cell into a tombstone (a key no lookup can ask for: keys are below 2^62).
// Afterwards the first insert is the only copy a lookup can match, wherever it sits -- and the
// ordinal it carries (cell word 3) names the key independently of the placement, which is what
// the per-sample seen-bitmap is indexed by.  A tombstone keeps its cell occupied and its
// fingerprint in the header, like the reference's unreachable duplicates keep theirs.  The first
// insert is never touched, so concurrent walkers always see it; each thread writes one word of
// its own cell only.
__global__ void kid_build_firstwins_kernel(uint4 *table, uint32_t slot_mask, const uint64_t *keys, const uint32_t *targets,
                                           uint64_t n, int k, uint32_t minloc, uint32_t line_shift, uint32_t line_mask)
{
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < n; e += (uint64_t)gridDim.x * blockDim.x) {
        if (targets[e] == 0 || table == nullptr) continue;
        const uint64_t key = keys[e];
        uint32_t my_idx = 0, min_ord = 0xFFFFFFFFu, copies = 0;
        if (minloc) {
            uint32_t line = kid_minloc_line(kid_minimizer_of_key(key, k), line_shift);
            for (;;) {
                const uint32_t base = line * KID_LINE_CELLS;
                const uint32_t w3 = reinterpret_cast<const uint32_t *>(table + base)[3];
                const uint32_t cnt = kid_hdr_count(w3);
                const uint32_t ne = cnt < KID_LINE_ENTRIES ? cnt : KID_LINE_ENTRIES;
                for (uint32_t j = 0; j < ne; j++) {
                    const uint32_t *c = reinterpret_cast<const uint32_t *>(table + base + 1u + j);
                    if (c[0] == (uint32_t)key && c[1] == (uint32_t)(key >> 32)) {
                        const uint32_t ord = c[3];
                        if (ord == (uint32_t)e + 1u) my_idx = base + 1u + j;
                        min_ord = ord < min_ord ? ord : min_ord;
                        copies++;
                    }
                }
                if (!kid_hdr_continues(w3, kid_key_fp(key))) break; // (every copy of this key left its trace on the way)
                line = (line + 1u) & line_mask;
            }
        } else {
            const uint32_t h = (uint32_t)kid_fmix64(key) & slot_mask;
            uint32_t rp = 0, i = 0;
            for (;;) {
                const uint32_t idx = (h + rp) & slot_mask;
                rp += ++i;
                const uint32_t *c = reinterpret_cast<const uint32_t *>(table + idx);
                const uint32_t ord = c[3];
                if (ord == 0) break;
                if (c[0] == (uint32_t)key && c[1] == (uint32_t)(key >> 32)) {
                    if (ord == (uint32_t)e + 1u) my_idx = idx;
                    min_ord = ord < min_ord ? ord : min_ord;
                    copies++;
                }
            }
        }
        if (copies > 1 && min_ord != (uint32_t)e + 1u) reinterpret_cast<uint32_t *>(table + my_idx)[1] = KID_TOMBSTONE_HI;
    }
}
