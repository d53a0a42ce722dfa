// kid_calls.hip.h -- the loop of the kernels that turn a hit list into one record per unit: kid_calls_run, compiled once per
// pair of a UNITS policy (what a unit is: a read of a CSR -- KidCsrUnits here -- or a segment, KidSegmentUnits of
// kid_segments.hip.h) and a METHOD policy (what is made of a unit's hits: Kid{Support,Vote,Loci}Method beside their kernels).
// Both are chosen by the kernel at compile time; nothing at run time selects a family, and what a pair does not use is not
// instantiated.  Four kernels are calls of it: kid_vote_kernel, kid_loci_kernel, kid_segments_kernel and
// kid_segment_votes_kernel.  Three carry the same loop written out, each for a figure its header gives, and must follow a
// change made here: kid_support_kernel, kid_fragment_kernel (timing) and kid_fragment_vote_kernel (registers).
//
// Work split: a wave takes 64 consecutive units and strides on by the grid.  A lane takes a unit of 1 .. lane_hits hits.
// Units of more are then taken by the whole wave one after the other, in the order of their lanes; where the method has a
// wave_hits, units of more than that are appended to a device list instead, for the family's second kernel: nothing is
// written and nothing is tallied for them here.  Every output word has one writer: the lane of the unit, or that kernel.
// Wave-uniform: the loop's bounds, what Units::span returns, and every argument and result of Method::wave.
//
// UNITS provides
//   hits                   the hit array the units' h0 count in
//   Unit                   at least {h0, m, n_kmers}: first hit, hits, windows; what else the record or the method needs
//   count()                units of the batch (uniform); 0 when nothing may be written
//   span(u0, n)            uniform work in front of the 64 lanes' own find (the segments' two searches; else nothing)
//   find(span, u, un)      lane: unit u -> un (un arrives zeroed and stays so for a lane without a unit)
//   counted(tally, u)      does a tally count unit u (TALLY kernels alone)
//   append(u, un)          unit u to the list (methods with a wave_hits alone)
//   store(u, un, res)      the unit's record
// METHOD provides
//   Result                 the record without the units' own fields; .confident where a kernel tallies
//   lane_hits, wave_hits   the two limits; wave_hits 0: the wave takes every wider unit, there is no list
//   empty(n_kmers, m)      the Result of a unit before its hits are looked at: what a unit without hits keeps
//   lane(h, un, res)       one lane, the un.m hits at h
//   wave(h, m, un, j, lane, res)  the whole wave, the m hits at h of lane j's unit (h, m uniform; un is each lane's own)
// The TALLY form counts the batch into a sample as if it had been classified under the rule: gcount[confident]++ per
// counted unit, and for units with confident > 0 kid_support_tally_hit on every hit (plain global atomics).
#pragma once
#include "kid_tile.hip.h"
#include "kid_hits.hip.h"
#include "kid_depth.hip.h"

struct KidSupportTally {
    unsigned long long *gcount;
    uint32_t *seen;
    // the descriptors of a FASTQ block's hit pass: a record process_qual dropped has n_kmers == 0 there and is counted
    // nowhere (a kept one has stop - start >= k, i.e. at least two windows).  null: every read of the batch is counted,
    // one shorter than k under target 0.
    const KidReadDesc *fastq_desc;
    uint32_t *depth; // the DEPTH form alone: one saturating counter per entry
};

// what a tally does with one hit of a unit it counted with confident > 0: the seen bit of a hit with target > 1, and in
// the DEPTH form (KID_OPT_ENTRY_DEPTH) 1 more on depth[entry] beside it (kid_depth.hip.h)
template <bool DEPTH>
__device__ __forceinline__ void kid_support_tally_hit(const KidSupportTally &tally, const KidHit &h)
{
    if (h.target > 1) {
        atomicOr(&tally.seen[h.entry >> 5], 1u << (h.entry & 31u));
        if (DEPTH) kid_depth_count(tally.depth, h.entry);
    }
}

struct KidNoSpan {};

// the reads of a hit CSR (the one kid_hits.hip.h leaves on the device, or the caller's).  list, n_list: uint32[n] and its
// length, zeroed in front of the kernel.
template <class Out>
struct KidCsrUnits {
    const uint64_t *hit_offsets;
    const KidHit *hits;
    const uint32_t *n_kmers;
    uint64_t n;
    Out *out; // nullable
    uint32_t *list, *n_list;
    struct Unit {
        uint64_t h0;
        uint32_t m, n_kmers;
    };
    __device__ __forceinline__ uint64_t count() const { return n; }
    __device__ __forceinline__ KidNoSpan span(uint64_t, uint64_t) const { return KidNoSpan(); }
    __device__ __forceinline__ void find(KidNoSpan, uint64_t u, Unit &un) const
    {
        un.h0 = hit_offsets[u];
        un.m = (uint32_t)(hit_offsets[u + 1] - un.h0);
        un.n_kmers = n_kmers[u];
    }
    __device__ __forceinline__ bool counted(const KidSupportTally &tally, uint64_t u) const
    {
        return !tally.fastq_desc || tally.fastq_desc[u].n_kmers > 0;
    }
    __device__ __forceinline__ void append(uint64_t u, const Unit &) const { list[atomicAdd(n_list, 1u)] = (uint32_t)u; }
    __device__ __forceinline__ void store(uint64_t u, const Unit &, const Out &res) const
    {
        if (out) out[u] = res;
    }
};

// the body of a kernel of 256 threads
template <bool TALLY, bool DEPTH, class Units, class Method>
__device__ __forceinline__ void kid_calls_run(const Units &U, const Method &M, const KidSupportTally &tally)
{
    constexpr bool LIST = Method::wave_hits != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_units = U.count(), n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t u0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; u0 < n_units; u0 += n_waves * 64u) {
        const auto span = U.span(u0, n_units);
        const uint64_t u = u0 + lane;
        const bool have = u < n_units;
        typename Units::Unit un = {};
        if (have) U.find(span, u, un);
        const uint32_t m = un.m;
        typename Method::Result res = Method::empty(un.n_kmers, m);
        bool later = false, counted = false;
        if constexpr (LIST) {
            later = m > Method::wave_hits;
            if (later) U.append(u, un);
        }
        if constexpr (TALLY) counted = have && !later && U.counted(tally, u);
        if (m > 0 && m <= Method::lane_hits) {
            M.lane(U.hits + un.h0, un, res);
            if constexpr (TALLY)
                if (counted && res.confident > 0)
                    for (uint32_t i = 0; i < m; i++) kid_support_tally_hit<DEPTH>(tally, U.hits[un.h0 + i]);
        }
        uint64_t wide = __ballot(m > Method::lane_hits && !later);
        while (wide) {
            const int j = __builtin_ctzll(wide);
            wide &= wide - 1ull;
            const KidHit *wh = U.hits + (uint64_t)__shfl((unsigned long long)un.h0, j);
            const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane((int)m, j);
            typename Method::Result w = Method::empty((uint32_t)__builtin_amdgcn_readlane((int)un.n_kmers, j), wm);
            M.wave(wh, wm, un, j, lane, w);
            if constexpr (TALLY)
                if (w.confident > 0 && ((__ballot(counted) >> j) & 1ull))
                    for (uint32_t c0 = 0; c0 < wm; c0 += 64u)
                        if (lane < wm - c0) kid_support_tally_hit<DEPTH>(tally, wh[(uint64_t)c0 + lane]);
            if (lane == (uint32_t)j) res = w;
        }
        if (have && !later) U.store(u, un, res);
        if constexpr (TALLY) {
            const uint64_t zeros = __ballot(counted && res.confident == 0); // half of a metagenomic sample: one add per wave
            if (lane == 0 && zeros) atomicAdd(&tally.gcount[0], (unsigned long long)__popcll(zeros));
            if (counted && res.confident != 0) atomicAdd(&tally.gcount[res.confident], 1ull);
        }
    }
}
