// kid_api_loci.h -- place reads on a genome by colinear hits: kid_db_set_sites and kid_db_read_loci* over the hit pass and
// the two kernels of kid_loci.hip.h -- and, once, the call path of the families that place by the database's sites
// (kid_loci_*<F>): the argument checks, the launch between the two events of the family's timer, the host run behind an
// opened batch and the two forms the families' extern "C" functions forward to (kid_loci_offsets, _from_hits_device).  A
// family is a struct like KidLociCalls below; the other is KidFragmentLociCalls (kid_api_fragment_loci.h), whose unit is
// two reads.  They have no rule, no tally and no sample, which is why they are not families of kid_calls_*
// (kid_api_support.h).  The sites are two uint32 per entry in HBM and belong to the kid_db; a family's scratch (a
// KidLociScratch of its own in the database's KidHitsState) grows with the largest batch, never with the table; a call waits
// for the kernels of its family's call before it (F::settle), and for nobody else's, before it binds the list again.
// Included behind kid_api_hits.h.
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

// A family of these calls is a struct with
//   Rec, id, unit_reads, settle   as in kid_api_support.h
//   Par                           its parameters: diag_bin, and what else its kernels' rule is made of
//   refusals                      the order in which a call is refused (kid_loci_check_args), as callers have always seen it
//   big, big_per_cu               its KidLociScratch in KidHitsState; the second kernel's workgroups per CU
//   args()                        what its kernels take between the CSR and `out`
//   kernel(), big_kernel()        the two kernels
struct KidLociPar {
    uint32_t diag_bin;
};
static KidLociSites kid_loci_sites(const kid_db *db, uint32_t diag_bin)
{
    return KidLociSites{db->sites->org.as<uint32_t>(), db->sites->pos.as<uint32_t>(), db->info.n_entries, diag_bin};
}
struct KidLociCalls {
    typedef KidLocus Rec;
    typedef KidLociPar Par;
    static constexpr KidFamily id = KID_FAM_LOCI;
    static constexpr uint64_t unit_reads = 1;
    static constexpr unsigned settle = kid_settle(KID_FAM_LOCI);
    static constexpr char refusals[] = "bnso"; // the checks of kid_db_read_support* with diag_bin in the place of the rule, then the sites
    static constexpr KidLociScratch KidHitsState::*big = &KidHitsState::loci_big;
    static constexpr unsigned big_per_cu = 4;
    static auto args(const kid_db *db, Par p) { return std::make_tuple(kid_loci_sites(db, p.diag_bin)); }
    static constexpr auto kernel() { return &kid_loci_kernel; }
    static constexpr auto big_kernel() { return &kid_loci_big_kernel; }
};

// what every form of a family refuses first, in the family's order: b diag_bin = 0, n the number of reads, o a null
// `out`, s a database without sites
template <class F> static int kid_loci_check_args(kid_db *db, uint64_t n_reads, uint32_t diag_bin, const void *out)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    for (const char c : F::refusals) {
        int rc = KID_OK;
        if (c == 'b' && diag_bin == 0) rc = kid_fail(KID_ERR_ARG, "diag_bin = 0: the diagonal bin is at least 1 wide");
        if (c == 'n' && (rc = kid_check_n_reads(n_reads)) == KID_OK && n_reads % F::unit_reads)
            rc = kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
        if (c == 'o' && n_reads && !out) rc = kid_fail(KID_ERR_ARG, "null argument");
        // (a look without hits_mu, like the other families' checks, so that the refusal does not wait behind a host-form call
        //  in flight; kid_loci_launch looks again under the lock before it hands the pointers to a kernel)
        if (c == 's') rc = kid_loci_check_sites(db);
        if (rc != KID_OK) return rc;
    }
    return KID_OK;
}

// The units of a batch bound to a family's scratch on `stream`: a list of n of them, none on it.
static int kid_loci_scratch_bind(KidLociScratch &s, uint64_t n, hipStream_t stream)
{
    KID_HIP(kid_hits_ensure(s.list, n * 4u));
    if (!s.n_list.p) KID_HIP(s.n_list.alloc(4));
    KID_HIP(hipMemsetAsync(s.n_list.p, 0, 4, stream));
    return KID_OK;
}

// the family's two kernels over one batch of n units on `stream` between the family's two events (under hits_mu)
template <class F>
static int kid_loci_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers, uint64_t n,
                           typename F::Par par, typename F::Rec *d_out, hipStream_t stream)
{
    int rc = kid_loci_check_sites(db);
    if (rc != KID_OK) return rc;
    KidLociScratch &s = h->*F::big;
    KidSpanTimer &timer = h->family[F::id].timer;
    if ((rc = timer.begin(stream)) != KID_OK) return rc;
    if ((rc = kid_loci_scratch_bind(s, n, stream)) != KID_OK) return rc;
    const KidLociBig big{s.list.as<uint32_t>(), s.n_list.as<uint32_t>()};
    std::apply(
        [&](auto... a) {
            hipLaunchKernelGGL(F::kernel(), dim3(kid_grid_for(n, 256, db->num_cu * 8)), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers, n,
                               a..., d_out, big);
            // (F::big_per_cu workgroups per CU for the units of the list, whose length the device alone knows: without any,
            //  the kernel returns at once)
            hipLaunchKernelGGL(F::big_kernel(), dim3(db->num_cu * F::big_per_cu), dim3(256), 0, stream, d_hit_offsets, d_hits, d_n_kmers, n, a...,
                               d_out, big);
        },
        F::args(db, par));
    KID_HIP(hipGetLastError());
    return timer.end(stream, n);
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch, the two kernels, one record per
// unit back.
template <class F> static int kid_loci_host_run(kid_db *db, const KidOpenBatch &ob, typename F::Par par, void *out)
{
    KidHitsState *h = ob.h;
    KidDevBuf &d_out = h->family[F::id].out;
    const uint64_t n = ob.b.n / F::unit_reads, out_nbytes = n * sizeof(typename F::Rec);
    uint64_t total = 0;
    int rc;
    KID_HIP(kid_hits_ensure(d_out, out_nbytes));
    if ((rc = kid_hits_host_pass(db, ob, KID_HITS_NO_LIMIT, &total)) != KID_OK) return rc;
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    rc = kid_loci_launch<F>(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), n, par,
                            d_out.as<typename F::Rec>(), 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(0));
    KID_HIP(hipMemcpy(out, d_out.p, out_nbytes, hipMemcpyDeviceToHost));
    return KID_OK;
}

// The forms both families have, once.  A batch of reads in host memory:
template <class F>
static int kid_loci_offsets(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop, uint64_t n_reads,
                            typename F::Par par, void *out)
{
    int rc = kid_loci_check_args<F>(db, n_reads, par.diag_bin, out);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, F::settle)) != KID_OK) return rc;
    return kid_loci_host_run<F>(db, ob, par, out);
}

// the family's kernels over a hit CSR in device memory (the caller's, or what kid_db_read_hits_device left)
template <class F>
static int kid_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                     typename F::Par par, void *d_out, void *stream)
{
    int rc = kid_loci_check_args<F>(db, n_reads, par.diag_bin, d_out);
    if (rc != KID_OK) return rc;
    if (n_reads && (!d_hit_offsets || !d_n_kmers)) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, F::settle, &h)) != KID_OK) return rc;
    return kid_loci_launch<F>(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers, n_reads / F::unit_reads,
                              par, (typename F::Rec *)d_out, (hipStream_t)stream);
}

extern "C" int kid_db_read_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                uint64_t n_reads, uint32_t diag_bin, kid_locus *out)
{
    return kid_loci_offsets<KidLociCalls>(db, bases, offsets, start, stop, n_reads, {diag_bin}, out);
}

extern "C" int kid_db_read_loci_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                      uint32_t diag_bin, kid_locus *out)
{
    int rc = kid_loci_check_args<KidLociCalls>(db, n_reads, diag_bin, out);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, KidLociCalls::settle)) != KID_OK) return rc;
    return kid_loci_host_run<KidLociCalls>(db, ob, {diag_bin}, out);
}

extern "C" int kid_db_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                            uint32_t diag_bin, void *d_out, void *stream)
{
    return kid_loci_from_hits_device<KidLociCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, {diag_bin}, d_out, stream);
}

extern "C" int kid_db_read_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KidLociCalls::id, device_ms, calls, reads);
}
