// kid_api_fragments.h -- call mate pairs as one fragment: kid_db_read_fragments* over the hit pass and kid_fragment_kernel
// (kid_fragments.hip.h).  The batch is 2 F reads in interleaved order (read 2i = mate 1 of fragment i, read 2i + 1 = its
// mate 2).  Everything but the kernel is shared: the family is KidFragmentCalls on the call path of kid_api_support.h
// (kid_calls_*: checks, host run, tally binding, launch, the four forms), the batch is opened by kid_hits_open_*
// (kid_api_hits.h), whose FASTQ form takes the two text blocks and stages them as one for one hit pass; the calls obey
// the one-call-at-a-time rule of every call on a kid_db.  The fragment kernel has the KidSpanTimer of the family's
// KidFamilyState in the database's KidHitsState.  Included behind kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_fragments.hip.h"

static_assert(sizeof(kid_fragment) == sizeof(KidFragment), "kid_fragment is the device record");

struct KidFragmentCalls {
    typedef KidFragment Rec;
    static constexpr KidFamily id = KID_FAM_FRAGMENTS;
    static constexpr uint64_t unit_reads = 2;
    static constexpr bool needs_sink = true;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT) | kid_settle(KID_FAM_FRAGMENTS);
    static constexpr KidVoteScratch KidHitsState::*big = nullptr;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_fragment_kernel<ROWS, TALLY, DEPTH>; }
};

extern "C" int kid_db_read_fragments(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                     uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment *out, kid_sample *tally)
{
    return kid_calls_offsets<KidFragmentCalls>(db, bases, offsets, start, stop, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_read_fragments_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                           uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t min_hits,
                                           uint32_t min_permille, kid_fragment *out, kid_sample *tally)
{
    return kid_calls_fastq_pairs<KidFragmentCalls>(db, text1, nbytes1, recs1, text2, nbytes2, recs2, n_fragments, min_hits, min_permille, out,
                                                   tally);
}

extern "C" int kid_db_fragments_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                 uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidFragmentCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_fragments_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, KidFragmentCalls::id, device_ms, calls, fragments);
}
