// kid_api_loci.h -- place reads on a genome by colinear hits: kid_db_set_sites and kid_db_read_loci* over the hit pass and
// the two kernels of kid_loci.hip.h.  The family has no rule, no tally and no sample, so it does not go through
// kid_calls_* (kid_api_support.h); what its forms share is here once: the checks (kid_loci_check_args), the launch
// between the two events of its timer (kid_loci_launch: the list of reads with more than KID_LOCI_WAVE_HITS hits and its
// length in the database's KidHitsState, kid_loci_kernel and kid_loci_big_kernel queued behind each other) and the host
// run behind an opened batch (kid_loci_host_run).  The sites are two uint32 per entry in HBM and belong to the kid_db; the
// scratch grows with the largest batch, never with the table; a call waits for the loci kernels of the call before it
// (kid_settle(KID_FAM_LOCI)) before it binds the list again.  Included behind kid_api_hits.h.
#pragma once
#include "kid_api_hits.h"
#include "kid_loci.hip.h"

static_assert(sizeof(kid_locus) == sizeof(KidLocus) && sizeof(KidLocus) == 40, "kid_locus is the device record");

extern "C" int kid_db_set_sites(kid_db *db, const uint32_t *org, const uint32_t *pos, uint64_t n_entries)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    const bool clear = !org && !pos && n_entries == 0;
    uint32_t n_orgs = 0;
    if (!clear) {
        if (!org || !pos) return kid_fail(KID_ERR_ARG, "null argument");
        if (n_entries != db->info.n_entries)
            return kid_fail(KID_ERR_ARG, "sites for %llu entries, the database has %llu", (unsigned long long)n_entries,
                            (unsigned long long)db->info.n_entries);
        for (uint64_t o = 0; o < n_entries; o++) {
            if (org[o] >= KID_LOCI_MAX_ORGS) return kid_fail(KID_ERR_ARG, "entry %llu: org = %u is 2^24 or more", (unsigned long long)o, org[o]);
            if (pos[o] >> 31) return kid_fail(KID_ERR_ARG, "entry %llu: pos = %u is 2^31 or more", (unsigned long long)o, pos[o]);
            n_orgs = org[o] >= n_orgs ? org[o] + 1u : n_orgs;
        }
    }
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    std::shared_ptr<KidSites> sites;
    if (!clear) { // (the old sites stay in force unless both copies arrive)
        sites = std::make_shared<KidSites>();
        sites->n_orgs = n_orgs;
        KID_HIP(sites->org.alloc(n_entries * 4));
        KID_HIP(sites->pos.alloc(n_entries * 4));
        KID_HIP(hipMemcpy(sites->org.p, org, n_entries * 4, hipMemcpyHostToDevice));
        KID_HIP(hipMemcpy(sites->pos.p, pos, n_entries * 4, hipMemcpyHostToDevice));
    }
    KID_HIP(hipDeviceSynchronize()); // no kernel of a device-form call still reads the sites that go
    db->sites = std::move(sites);    // (a pileup made from the old ones keeps them: kid_api_pileup.h)
    db->sites_gen++;
    return KID_OK;
}

static int kid_loci_check_sites(kid_db *db)
{
    if (!db->sites) return kid_fail(KID_ERR_STATE, "the database has no sites (kid_db_set_sites)");
    return KID_OK;
}

// what every form refuses first, in the order callers see: the checks of kid_db_read_support* with diag_bin in the
// place of the rule, then a database without sites
static int kid_loci_check_args(kid_db *db, uint64_t n_reads, uint32_t diag_bin, const void *out)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    if (diag_bin == 0) return kid_fail(KID_ERR_ARG, "diag_bin = 0: the diagonal bin is at least 1 wide");
    int rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    // (a look without hits_mu, like the other families' checks, so that the refusal does not wait behind a host-form call
    //  in flight; kid_loci_launch looks again under the lock before it hands the pointers to a kernel)
    if ((rc = kid_loci_check_sites(db)) != KID_OK) return rc;
    if (n_reads && !out) return kid_fail(KID_ERR_ARG, "null argument");
    return KID_OK;
}

// the two kernels over one batch of n reads on `stream` between the family's two events (under hits_mu)
static int kid_loci_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers, uint64_t n,
                           uint32_t diag_bin, KidLocus *d_out, hipStream_t stream)
{
    int rc = kid_loci_check_sites(db);
    if (rc != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->loci_list, n * 4u));
    if (!h->loci_n_list.p) KID_HIP(h->loci_n_list.alloc(4));
    const KidLociSites sites{db->sites->org.as<uint32_t>(), db->sites->pos.as<uint32_t>(), db->info.n_entries, diag_bin};
    const KidLociBig big{h->loci_list.as<uint32_t>(), h->loci_n_list.as<uint32_t>()};
    KidSpanTimer &timer = h->family[KID_FAM_LOCI].timer;
    if ((rc = timer.begin(stream)) != KID_OK) return rc;
    KID_HIP(hipMemsetAsync(big.n_list, 0, 4, stream));
    hipLaunchKernelGGL(kid_loci_kernel, dim3(kid_grid_for(n, 256, db->num_cu * 8)), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers, n,
                       sites, d_out, big);
    // (one workgroup per read of the list, whose length the device alone knows: without any, the kernel returns at once)
    hipLaunchKernelGGL(kid_loci_big_kernel, dim3(db->num_cu * 4), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers, n, sites, d_out, big);
    KID_HIP(hipGetLastError());
    return timer.end(stream, n);
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch, the two kernels, one record per
// read back.
static int kid_loci_host_run(kid_db *db, const KidOpenBatch &ob, uint32_t diag_bin, kid_locus *out)
{
    KidHitsState *h = ob.h;
    KidDevBuf &d_out = h->family[KID_FAM_LOCI].out;
    const uint64_t n = ob.b.n;
    uint64_t total = 0;
    int rc;
    KID_HIP(kid_hits_ensure(d_out, n * sizeof(KidLocus)));
    if ((rc = kid_hits_host_pass(db, ob, KID_HITS_NO_LIMIT, &total)) != KID_OK) return rc;
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    rc = kid_loci_launch(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), n, diag_bin,
                         d_out.as<KidLocus>(), 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(0));
    KID_HIP(hipMemcpy(out, d_out.p, n * sizeof(KidLocus), hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_db_read_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                uint64_t n_reads, uint32_t diag_bin, kid_locus *out)
{
    int rc = kid_loci_check_args(db, n_reads, diag_bin, out);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, kid_settle(KID_FAM_LOCI))) != KID_OK) return rc;
    return kid_loci_host_run(db, ob, diag_bin, out);
}

extern "C" int kid_db_read_loci_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                      uint32_t diag_bin, kid_locus *out)
{
    int rc = kid_loci_check_args(db, n_reads, diag_bin, out);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, kid_settle(KID_FAM_LOCI))) != KID_OK) return rc;
    return kid_loci_host_run(db, ob, diag_bin, out);
}

extern "C" int kid_db_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                            uint32_t diag_bin, void *d_out, void *stream)
{
    int rc = kid_loci_check_args(db, n_reads, diag_bin, d_out);
    if (rc != KID_OK) return rc;
    if (n_reads && (!d_hit_offsets || !d_n_kmers)) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, kid_settle(KID_FAM_LOCI), &h)) != KID_OK) return rc;
    return kid_loci_launch(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers, n_reads, diag_bin,
                           (KidLocus *)d_out, (hipStream_t)stream);
}

extern "C" int kid_db_read_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KID_FAM_LOCI, device_ms, calls, reads);
}
