// kid_api_fragment_loci.h -- place mate pairs as one fragment by colinear hits: kid_db_read_fragment_loci* over the hit
// pass and the two kernels of kid_fragment_loci.hip.h.  The batch is 2 F reads in interleaved order, as for
// kid_db_read_fragments*; the forms mirror that quartet argument for argument with (diag_bin, max_span) in the place of the
// rule and without a tally.  The call path is that of kid_api_loci.h (kid_loci_*<F>) with the family below: a unit of two
// reads, the order of refusals of kid_db_read_fragments*, a list and a counter of its own, and an entry of its own
// (KID_FAM_FRAGMENT_LOCI): a call waits for the fragment-loci kernels of the call before it before it zeroes the list's
// counter, and for nobody else's.  Included behind kid_api_loci.h.
#pragma once
#include "kid_api_loci.h"
#include "kid_fragment_loci.hip.h"

static_assert(sizeof(kid_fragment_locus) == sizeof(KidFragmentLocus) && sizeof(KidFragmentLocus) == 64, "kid_fragment_locus is the device record");

struct KidFragmentLociPar {
    uint32_t diag_bin, max_span;
};
struct KidFragmentLociCalls {
    typedef KidFragmentLocus Rec;
    typedef KidFragmentLociPar Par;
    static constexpr KidFamily id = KID_FAM_FRAGMENT_LOCI;
    static constexpr uint64_t unit_reads = 2;
    static constexpr unsigned settle = kid_settle(KID_FAM_FRAGMENT_LOCI);
    // the checks of kid_db_read_fragments* (odd n_reads, null pointers), then diag_bin = 0, then a database without sites
    static constexpr char refusals[] = "nobs";
    static constexpr KidLociScratch KidHitsState::*big = &KidHitsState::fragment_loci_big;
    static constexpr unsigned big_per_cu = 2; // (two workgroups of 64 KiB of LDS fit a CU)
    static auto args(const kid_db *db, Par p)
    {
        return std::make_tuple(kid_loci_sites(db, p.diag_bin), KidFlociRule{p.max_span / p.diag_bin, (uint32_t)db->info.k});
    }
    static constexpr auto kernel() { return &kid_fragment_loci_kernel; }
    static constexpr auto big_kernel() { return &kid_fragment_loci_big_kernel; }
};

extern "C" int kid_db_read_fragment_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                         uint64_t n_reads, uint32_t diag_bin, uint32_t max_span, kid_fragment_locus *out)
{
    return kid_loci_offsets<KidFragmentLociCalls>(db, bases, offsets, start, stop, n_reads, {diag_bin, max_span}, out);
}

extern "C" int kid_db_read_fragment_loci_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                               uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t diag_bin,
                                               uint32_t max_span, kid_fragment_locus *out)
{
    typedef KidFragmentLociCalls F;
    // (the checks of kid_calls_fastq_pairs, in its order)
    if (n_fragments > 0x3FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^30-1 fragments per batch");
    int rc = kid_loci_check_args<F>(db, 2 * n_fragments, diag_bin, out);
    if (rc != KID_OK || n_fragments == 0) return rc;
    if (!recs1 || !recs2 || (!text1 && nbytes1) || (!text2 && nbytes2)) return kid_fail(KID_ERR_ARG, "null argument");
    if (nbytes1 + nbytes2 < nbytes1 || nbytes1 + nbytes2 >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "two FASTQ blocks of 4 GiB or more together");
    KidOpenBatch ob;
    rc = kid_hits_open_fastq(ob, db, text1, nbytes1, recs1, 2 * n_fragments, F::settle, nullptr, text2, nbytes2, recs2);
    if (rc != KID_OK) return rc;
    return kid_loci_host_run<F>(db, ob, {diag_bin, max_span}, out);
}

extern "C" int kid_db_fragment_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                     uint64_t n_reads, uint32_t diag_bin, uint32_t max_span, void *d_out, void *stream)
{
    return kid_loci_from_hits_device<KidFragmentLociCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, {diag_bin, max_span}, d_out, stream);
}

extern "C" int kid_db_read_fragment_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, KidFragmentLociCalls::id, device_ms, calls, fragments);
}
