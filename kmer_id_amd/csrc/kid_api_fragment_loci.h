// kid_api_fragment_loci.h -- place mate pairs as one fragment by colinear hits: kid_db_read_fragment_loci* over the hit
// pass and the two kernels of kid_fragment_loci.hip.h.  The batch is 2 F reads in interleaved order, as for
// kid_db_read_fragments*; the forms mirror that quartet argument for argument with (diag_bin, max_span) in the place of the
// rule and without a tally.  Like the loci family it has no rule, no tally and no sample, so it does not go through
// kid_calls_*; what its forms share is here once: the checks (kid_floci_check_args), the launch between the two events of
// its timer (kid_floci_launch: the list of fragments left to the second kernel and its length in the database's
// KidHitsState, the two kernels queued behind each other) and the host run behind an opened batch (kid_floci_host_run).
// The family has its own entry (KID_FAM_FRAGMENT_LOCI): a call waits for the fragment-loci kernels of the call before it
// before it zeroes the list's counter, and for nobody else's.  Included behind kid_api_loci.h.
#pragma once
#include "kid_api_loci.h"
#include "kid_fragment_loci.hip.h"

static_assert(sizeof(kid_fragment_locus) == sizeof(KidFragmentLocus) && sizeof(KidFragmentLocus) == 64, "kid_fragment_locus is the device record");

// what every form refuses first, in the order callers see: the checks of kid_db_read_fragments* (odd n_reads, null
// pointers), then diag_bin = 0, then a database without sites
static int kid_floci_check_args(kid_db *db, uint64_t n_reads, uint32_t diag_bin, const void *out)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (n_reads % 2u) return kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
    if (n_reads && !out) return kid_fail(KID_ERR_ARG, "null argument");
    if (diag_bin == 0) return kid_fail(KID_ERR_ARG, "diag_bin = 0: the diagonal bin is at least 1 wide");
    // (a look without hits_mu, as in kid_loci_check_args; kid_floci_launch looks again under the lock)
    return kid_loci_check_sites(db);
}

// the two kernels over one batch of n fragments on `stream` between the family's two events (under hits_mu)
static int kid_floci_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers, uint64_t n,
                            uint32_t diag_bin, uint32_t max_span, KidFragmentLocus *d_out, hipStream_t stream)
{
    int rc = kid_loci_check_sites(db);
    if (rc != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->fragment_loci_list, n * 4u));
    if (!h->fragment_loci_n_list.p) KID_HIP(h->fragment_loci_n_list.alloc(4));
    const KidLociSites sites{db->sites->org.as<uint32_t>(), db->sites->pos.as<uint32_t>(), db->info.n_entries, diag_bin};
    const KidFlociRule rule{max_span / diag_bin, (uint32_t)db->info.k};
    const KidLociBig big{h->fragment_loci_list.as<uint32_t>(), h->fragment_loci_n_list.as<uint32_t>()};
    KidSpanTimer &timer = h->family[KID_FAM_FRAGMENT_LOCI].timer;
    if ((rc = timer.begin(stream)) != KID_OK) return rc;
    KID_HIP(hipMemsetAsync(big.n_list, 0, 4, stream));
    hipLaunchKernelGGL(kid_fragment_loci_kernel, dim3(kid_grid_for(n, 256, db->num_cu * 8)), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers,
                       n, sites, rule, d_out, big);
    // (one workgroup per fragment of the list, whose length the device alone knows: without any, the kernel returns at
    //  once.  Two workgroups of 64 KiB of LDS fit a CU.)
    hipLaunchKernelGGL(kid_fragment_loci_big_kernel, dim3(db->num_cu * 2), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers, n, sites, rule,
                       d_out, big);
    KID_HIP(hipGetLastError());
    return timer.end(stream, n);
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch, the two kernels, one record per
// fragment back.
static int kid_floci_host_run(kid_db *db, const KidOpenBatch &ob, uint32_t diag_bin, uint32_t max_span, kid_fragment_locus *out)
{
    KidHitsState *h = ob.h;
    KidDevBuf &d_out = h->family[KID_FAM_FRAGMENT_LOCI].out;
    const uint64_t n = ob.b.n / 2u;
    uint64_t total = 0;
    int rc;
    KID_HIP(kid_hits_ensure(d_out, n * sizeof(KidFragmentLocus)));
    if ((rc = kid_hits_host_pass(db, ob, KID_HITS_NO_LIMIT, &total)) != KID_OK) return rc;
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    rc = kid_floci_launch(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), n, diag_bin,
                          max_span, d_out.as<KidFragmentLocus>(), 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(0));
    KID_HIP(hipMemcpy(out, d_out.p, n * sizeof(KidFragmentLocus), hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_db_read_fragment_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                         uint64_t n_reads, uint32_t diag_bin, uint32_t max_span, kid_fragment_locus *out)
{
    int rc = kid_floci_check_args(db, n_reads, diag_bin, out);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, kid_settle(KID_FAM_FRAGMENT_LOCI))) != KID_OK) return rc;
    return kid_floci_host_run(db, ob, diag_bin, max_span, out);
}

extern "C" int kid_db_read_fragment_loci_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                               uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t diag_bin,
                                               uint32_t max_span, kid_fragment_locus *out)
{
    // (the checks of kid_calls_fastq_pairs, in its order)
    if (n_fragments > 0x3FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^30-1 fragments per batch");
    int rc = kid_floci_check_args(db, 2 * n_fragments, diag_bin, out);
    if (rc != KID_OK || n_fragments == 0) return rc;
    if (!recs1 || !recs2 || (!text1 && nbytes1) || (!text2 && nbytes2)) return kid_fail(KID_ERR_ARG, "null argument");
    if (nbytes1 + nbytes2 < nbytes1 || nbytes1 + nbytes2 >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "two FASTQ blocks of 4 GiB or more together");
    KidOpenBatch ob;
    rc = kid_hits_open_fastq(ob, db, text1, nbytes1, recs1, 2 * n_fragments, kid_settle(KID_FAM_FRAGMENT_LOCI), nullptr, text2, nbytes2, recs2);
    if (rc != KID_OK) return rc;
    return kid_floci_host_run(db, ob, diag_bin, max_span, out);
}

extern "C" int kid_db_fragment_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                     uint64_t n_reads, uint32_t diag_bin, uint32_t max_span, void *d_out, void *stream)
{
    int rc = kid_floci_check_args(db, n_reads, diag_bin, d_out);
    if (rc != KID_OK) return rc;
    if (n_reads && (!d_hit_offsets || !d_n_kmers)) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, kid_settle(KID_FAM_FRAGMENT_LOCI), &h)) != KID_OK) return rc;
    return kid_floci_launch(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers, n_reads / 2u, diag_bin,
                            max_span, (KidFragmentLocus *)d_out, (hipStream_t)stream);
}

extern "C" int kid_db_read_fragment_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, KID_FAM_FRAGMENT_LOCI, device_ms, calls, fragments);
}
