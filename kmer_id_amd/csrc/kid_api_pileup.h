// kid_api_pileup.h -- placed reads piled up per genome bin: the kid_pileup handle over the kernels of kid_pileup.hip.h.
// A pileup is made from a database's sites and a bin width: it shares the two site arrays with the kid_db (KidSites, so a
// later kid_db_set_sites or kid_db_destroy frees nothing a queued kernel or a later call of the pileup reads) and owns its
// geometry (span_bins, bin_base: the kernels of kid_coverage.hip.h), the two accumulators (`starts` [B], the step array
// [B + n_orgs]), two 64-bit counts and the scratch of a summary (the scanned steps, the tile sums, the records).  Device
// memory: 12 bytes per organism and 12 bytes per bin for good, 48 per organism more from the first summary and 4 per bin
// more from the first kid_pileup_bins; at KID_COVERAGE_MAX_BINS about 3 GiB (4 with kid_pileup_bins).
// kid_pileup_add_device queues one kernel on the caller's stream between two events of its own; the reading calls wait for
// every such pair (which is also where the device time comes from), then scan and reduce on the null stream.  The add
// kernel only adds, so adds on several streams run beside each other.  Calls on one pileup are serialised by its mutex.
// Included behind kid_api_loci.h.
#pragma once
#include <memory>
#include <mutex>
#include <stddef.h>
#include <vector>

#include "kid_api_loci.h"
#include "kid_pileup.hip.h"

static_assert(sizeof(kid_pileup_rec) == 48 && offsetof(kid_pileup_rec, reserved) == 32 && offsetof(kid_pileup_rec, depth_sum) == 40 &&
                  sizeof(kid_pileup_rec) == KID_PILEUP_REC_WORDS * 4,
              "kid_pileup_rec is the device record: nine uint32, four bytes of padding, one uint64");

struct kid_pileup {
    kid_db *db = nullptr; // for the generation of its sites alone; never touched by kid_pileup_destroy
    int device = 0, num_cu = 0;
    uint64_t gen = 0;                // db->sites_gen when the pileup was made
    std::shared_ptr<KidSites> sites; // the sites the geometry is of
    uint32_t n_orgs = 0, bin_width = 0, k = 0;
    uint64_t n_entries = 0, n_bins = 0, n_slots = 0, n_tiles = 0;
    KidDevBuf span, bin_base;   // uint32 [n_orgs], unsigned long long [n_orgs + 1]
    KidDevBuf starts, steps;    // uint32 [n_bins], uint32 [n_slots]
    KidDevBuf counts;           // unsigned long long [2]: records handed in, records placed
    KidDevBuf depth, tile_sums; // the scan: uint32 [n_slots], uint32 [n_tiles]
    KidDevBuf recs, depth_bins; // made when first asked for: KID_PILEUP_REC_WORDS words per organism, uint32 [n_bins]
    KidDevBuf staged;           // the records of kid_pileup_add, the arrays of kid_pileup_merge (grow-only)
    uint64_t merged_records = 0, merged_placed = 0; // what kid_pileup_merge added since the last reset
    struct Span {
        KidEvent ev0, ev1;
    };
    std::vector<Span> queued, spare; // around every add kernel not yet waited for; events to use again
    double ms = 0;
    uint64_t calls = 0, records = 0;
    std::mutex mu;
};

// every queued add is through, its device time taken (under mu)
static int kid_pileup_settle(kid_pileup *p)
{
    while (!p->queued.empty()) {
        kid_pileup::Span &s = p->queued.back();
        KID_HIP(hipEventSynchronize(s.ev1.e));
        float span = 0;
        KID_HIP(hipEventElapsedTime(&span, s.ev0.e, s.ev1.e));
        p->ms += span;
        p->spare.push_back(std::move(s));
        p->queued.pop_back();
    }
    return KID_OK;
}

static KidPileupGeo kid_pileup_geo(const kid_pileup *p)
{
    return KidPileupGeo{p->sites->org.as<uint32_t>(), p->sites->pos.as<uint32_t>(), p->n_entries, p->span.as<uint32_t>(),
                        p->bin_base.as<unsigned long long>(), p->n_orgs, p->bin_width, p->k};
}

extern "C" int kid_pileup_destroy(kid_pileup *p)
{
    if (!p) return kid_fail(KID_ERR_ARG, "null argument");
    hipSetDevice(p->device); // the owners' destructors free on the current device
    hipDeviceSynchronize();  // nothing of the pileup goes while a kernel may still use it
    delete p;
    return KID_OK;
}

extern "C" int kid_pileup_create(kid_db *db, uint32_t bin_width, kid_pileup **out)
{
    if (!db || !out) return kid_fail(KID_ERR_ARG, "null argument");
    *out = nullptr;
    if (bin_width == 0) return kid_fail(KID_ERR_ARG, "bin_width is 0");
    std::unique_ptr<kid_pileup> p(new kid_pileup());
    {
        std::lock_guard<std::mutex> lock(db->hits_mu);
        int rc = kid_loci_check_sites(db);
        if (rc != KID_OK) return rc;
        p->sites = db->sites;
        p->gen = db->sites_gen;
    }
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    p->db = db;
    p->device = db->device;
    p->num_cu = db->num_cu;
    p->n_orgs = p->sites->n_orgs;
    p->bin_width = bin_width;
    p->k = (uint32_t)db->info.k;
    p->n_entries = db->info.n_entries;
    const uint32_t n_orgs = p->n_orgs;
    KID_HIP(p->span.alloc((size_t)n_orgs * 4));
    KID_HIP(p->bin_base.alloc(((size_t)n_orgs + 1) * 8));
    KID_HIP(p->counts.alloc(16));
    KID_HIP(hipMemset(p->span.p, 0, p->span.cap));
    KID_HIP(hipMemset(p->counts.p, 0, 16));
    if (p->n_entries)
        hipLaunchKernelGGL(kid_cov_span_kernel, dim3(kid_grid_for(p->n_entries, 256, p->num_cu * 8)), dim3(256), 0, 0, p->sites->org.as<uint32_t>(),
                           p->sites->pos.as<uint32_t>(), p->n_entries, n_orgs, bin_width, p->span.as<uint32_t>());
    hipLaunchKernelGGL(kid_cov_scan_kernel, dim3(1), dim3(256), 0, 0, p->span.as<uint32_t>(), n_orgs, p->bin_base.as<unsigned long long>());
    KID_HIP(hipGetLastError());
    uint64_t B = 0;
    KID_HIP(hipMemcpy(&B, p->bin_base.as<unsigned long long>() + n_orgs, 8, hipMemcpyDeviceToHost));
    if (B > KID_COVERAGE_MAX_BINS) {
        rc = kid_fail(KID_ERR_ARG, "%llu bins of %u bases over all organisms: more than KID_COVERAGE_MAX_BINS", (unsigned long long)B, bin_width);
        (void)kid_pileup_destroy(p.release());
        return rc;
    }
    p->n_bins = B;
    p->n_slots = B + n_orgs;
    p->n_tiles = (p->n_slots + KID_PILEUP_SCAN_TILE - 1) / KID_PILEUP_SCAN_TILE;
    hipError_t e = p->starts.alloc((size_t)B * 4);
    if (e == hipSuccess) e = p->steps.alloc((size_t)p->n_slots * 4);
    if (e == hipSuccess) e = p->depth.alloc((size_t)p->n_slots * 4);
    if (e == hipSuccess) e = p->tile_sums.alloc((size_t)p->n_tiles * 4);
    if (e == hipSuccess) e = hipMemset(p->starts.p, 0, p->starts.cap);
    if (e == hipSuccess) e = hipMemset(p->steps.p, 0, p->steps.cap);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)kid_pileup_destroy(p.release());
        KID_HIP(e);
    }
    *out = p.release();
    return KID_OK;
}

extern "C" int kid_pileup_info(kid_pileup *p, uint32_t *n_orgs, uint64_t *n_bins, uint32_t *bin_width)
{
    if (!p) return kid_fail(KID_ERR_ARG, "null argument");
    if (n_orgs) *n_orgs = p->n_orgs;
    if (n_bins) *n_bins = p->n_bins;
    if (bin_width) *bin_width = p->bin_width;
    return KID_OK;
}

extern "C" int kid_pileup_reset(kid_pileup *p)
{
    if (!p) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc;
    KID_HIP(hipMemset(p->starts.p, 0, p->starts.cap));
    KID_HIP(hipMemset(p->steps.p, 0, p->steps.cap));
    KID_HIP(hipMemset(p->counts.p, 0, 16));
    KID_HIP(hipDeviceSynchronize());
    p->merged_records = p->merged_placed = 0;
    return KID_OK;
}

// what both forms of kid_pileup_add refuse, in the order callers see; *go: there is something to launch
static int kid_pileup_check_add(kid_pileup *p, const void *loci, uint64_t n, uint32_t min_chain, bool *go)
{
    *go = false;
    if (!p || (n && !loci)) return kid_fail(KID_ERR_ARG, "null argument");
    if (min_chain == 0) return kid_fail(KID_ERR_ARG, "min_chain = 0: a placed record has a chain");
    {
        std::lock_guard<std::mutex> lock(p->db->hits_mu);
        if (p->db->sites_gen != p->gen)
            return kid_fail(KID_ERR_STATE, "the database's sites were set again after this pileup was made: its geometry is stale");
    }
    if (n == 0) return KID_OK;
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    *go = true;
    return KID_OK;
}

// the add kernel over n records in HBM on `stream` between two events (under mu)
template <class Rec>
static int kid_pileup_launch_add(kid_pileup *p, const Rec *d_recs, uint64_t n, KidPileupRule rule, hipStream_t stream)
{
    if (p->queued.size() >= 64) { // (a caller that never reads: the events do not pile up)
        int rc = kid_pileup_settle(p);
        if (rc != KID_OK) return rc;
    }
    kid_pileup::Span s;
    if (!p->spare.empty()) {
        s = std::move(p->spare.back());
        p->spare.pop_back();
    } else {
        KID_HIP(s.ev0.create());
        KID_HIP(s.ev1.create());
    }
    KID_HIP(hipEventRecord(s.ev0.e, stream));
    hipLaunchKernelGGL(kid_pileup_add_kernel<Rec>, dim3(kid_grid_for(n, 256, p->num_cu * 8)), dim3(256), 0, stream, d_recs, n, kid_pileup_geo(p), rule,
                       p->starts.as<uint32_t>(), p->steps.as<uint32_t>(), p->counts.as<unsigned long long>());
    KID_HIP(hipGetLastError());
    KID_HIP(hipEventRecord(s.ev1.e, stream));
    p->queued.push_back(std::move(s));
    p->calls++;
    p->records += n;
    return KID_OK;
}

// the two forms of an add, for either record type: the records in HBM on the caller's stream, or staged from the host
template <class Rec>
static int kid_pileup_add_on_device(kid_pileup *p, const void *d_recs, uint64_t n, KidPileupRule rule, void *stream)
{
    bool go;
    int rc = kid_pileup_check_add(p, d_recs, n, rule.min_chain, &go);
    if (rc != KID_OK || !go) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    return kid_pileup_launch_add(p, (const Rec *)d_recs, n, rule, (hipStream_t)stream);
}

template <class Rec>
static int kid_pileup_add_from_host(kid_pileup *p, const void *recs, uint64_t n, KidPileupRule rule)
{
    bool go;
    int rc = kid_pileup_check_add(p, recs, n, rule.min_chain, &go);
    if (rc != KID_OK || !go) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc; // (the add before may still read the staged records)
    KID_HIP(kid_hits_ensure(p->staged, n * sizeof(Rec)));
    KID_HIP(hipMemcpy(p->staged.p, recs, n * sizeof(Rec), hipMemcpyHostToDevice));
    return kid_pileup_launch_add(p, p->staged.as<Rec>(), n, rule, 0);
}

extern "C" int kid_pileup_add_device(kid_pileup *p, const void *d_loci, uint64_t n, uint32_t min_chain, uint32_t min_margin, void *stream)
{
    return kid_pileup_add_on_device<KidLocus>(p, d_loci, n, KidPileupRule{min_chain, min_margin, 0u}, stream);
}

extern "C" int kid_pileup_add(kid_pileup *p, const kid_locus *loci, uint64_t n, uint32_t min_chain, uint32_t min_margin)
{
    return kid_pileup_add_from_host<KidLocus>(p, loci, n, KidPileupRule{min_chain, min_margin, 0u});
}

extern "C" int kid_pileup_add_fragments_device(kid_pileup *p, const void *d_recs, uint64_t n, uint32_t min_chain, uint32_t min_margin,
                                               int paired_only, void *stream)
{
    return kid_pileup_add_on_device<KidFragmentLocus>(p, d_recs, n, KidPileupRule{min_chain, min_margin, paired_only ? 1u : 0u}, stream);
}

extern "C" int kid_pileup_add_fragments(kid_pileup *p, const kid_fragment_locus *recs, uint64_t n, uint32_t min_chain, uint32_t min_margin,
                                        int paired_only)
{
    return kid_pileup_add_from_host<KidFragmentLocus>(p, recs, n, KidPileupRule{min_chain, min_margin, paired_only ? 1u : 0u});
}

extern "C" int kid_pileup_counts(kid_pileup *p, uint64_t *n_records, uint64_t *n_placed)
{
    if (!p) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc;
    unsigned long long c[2] = {0, 0};
    KID_HIP(hipMemcpy(c, p->counts.p, 16, hipMemcpyDeviceToHost));
    if (n_records) *n_records = c[0] + p->merged_records;
    if (n_placed) *n_placed = c[1] + p->merged_placed;
    return KID_OK;
}

// The three kernels of the scan and the reduce kernel on the null stream, behind every queued add (under mu).
// recs: the records are wanted; bins: depth in the layout of `starts` is.
static int kid_pileup_scan_reduce(kid_pileup *p, bool recs, bool bins)
{
    int rc = kid_pileup_settle(p);
    if (rc != KID_OK) return rc;
    if (recs && !p->recs.p) KID_HIP(p->recs.alloc((size_t)p->n_orgs * KID_PILEUP_REC_WORDS * 4));
    if (bins && !p->depth_bins.p) KID_HIP(p->depth_bins.alloc((size_t)p->n_bins * 4));
    const int grid = kid_grid_for(p->n_tiles, 1, p->num_cu * 8);
    if (p->n_tiles) {
        hipLaunchKernelGGL(kid_pileup_tile_sum_kernel, dim3(grid), dim3(256), 0, 0, p->steps.as<uint32_t>(), p->n_slots, p->n_tiles,
                           p->tile_sums.as<uint32_t>());
        hipLaunchKernelGGL(kid_pileup_tile_scan_kernel, dim3(1), dim3(256), 0, 0, p->tile_sums.as<uint32_t>(), p->n_tiles);
        hipLaunchKernelGGL(kid_pileup_apply_kernel, dim3(grid), dim3(256), 0, 0, p->steps.as<uint32_t>(), p->n_slots, p->n_tiles,
                           p->tile_sums.as<uint32_t>(), p->depth.as<uint32_t>());
    }
    if (p->n_orgs)
        hipLaunchKernelGGL(kid_pileup_reduce_kernel, dim3(kid_grid_for((uint64_t)p->n_orgs * 64, 256, p->num_cu * 16)), dim3(256), 0, 0,
                           p->span.as<uint32_t>(), p->bin_base.as<unsigned long long>(), p->starts.as<uint32_t>(), p->depth.as<uint32_t>(),
                           p->n_orgs, recs ? p->recs.as<uint32_t>() : nullptr, bins ? p->depth_bins.as<uint32_t>() : nullptr);
    KID_HIP(hipGetLastError());
    KID_HIP(hipStreamSynchronize(0));
    return KID_OK;
}

extern "C" int kid_pileup_summary(kid_pileup *p, kid_pileup_rec *out)
{
    if (!p || !out) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_scan_reduce(p, true, false)) != KID_OK) return rc;
    if (p->n_orgs) KID_HIP(hipMemcpy(out, p->recs.p, (size_t)p->n_orgs * sizeof(kid_pileup_rec), hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_pileup_bins(kid_pileup *p, uint64_t *bin_base, uint32_t *starts, uint32_t *depth, uint64_t cap)
{
    if (!p || !bin_base) return kid_fail(KID_ERR_ARG, "null argument");
    // both arrays, or neither and no room: the sizing call
    if ((starts == nullptr) != (depth == nullptr) || (!starts && cap != 0))
        return kid_fail(KID_ERR_ARG, "starts and depth go together, and without them cap is 0");
    if (starts && cap < p->n_bins)
        return kid_fail(KID_ERR_ARG, "room for %llu bins where there are %llu", (unsigned long long)cap, (unsigned long long)p->n_bins);
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if (starts) {
        if ((rc = kid_pileup_scan_reduce(p, false, true)) != KID_OK) return rc;
        if (p->n_bins) {
            KID_HIP(hipMemcpy(starts, p->starts.p, (size_t)p->n_bins * 4, hipMemcpyDeviceToHost));
            KID_HIP(hipMemcpy(depth, p->depth_bins.p, (size_t)p->n_bins * 4, hipMemcpyDeviceToHost));
        }
    }
    KID_HIP(hipMemcpy(bin_base, p->bin_base.p, ((size_t)p->n_orgs + 1) * 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_pileup_export(kid_pileup *p, uint32_t *starts, uint32_t *steps)
{
    if (!p || !starts || !steps) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc;
    if (p->n_bins) KID_HIP(hipMemcpy(starts, p->starts.p, (size_t)p->n_bins * 4, hipMemcpyDeviceToHost));
    if (p->n_slots) KID_HIP(hipMemcpy(steps, p->steps.p, (size_t)p->n_slots * 4, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_pileup_merge(kid_pileup *p, const uint32_t *starts, const uint32_t *steps, uint64_t n_records, uint64_t n_placed)
{
    if (!p || !starts || !steps) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc; // (a host-form add may still read `staged`)
    const struct { const uint32_t *src; KidDevBuf *dst; uint64_t n; } parts[2] = {{starts, &p->starts, p->n_bins}, {steps, &p->steps, p->n_slots}};
    for (const auto &part : parts) {
        if (part.n == 0) continue;
        KID_HIP(kid_hits_ensure(p->staged, part.n * 4));
        KID_HIP(hipMemcpy(p->staged.p, part.src, part.n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(kid_pileup_merge_kernel, dim3(kid_grid_for(part.n, 256, p->num_cu * 8)), dim3(256), 0, 0, p->staged.as<uint32_t>(), part.n,
                           part.dst->as<uint32_t>());
        KID_HIP(hipGetLastError());
        KID_HIP(hipStreamSynchronize(0));
    }
    p->merged_records += n_records;
    p->merged_placed += n_placed;
    return KID_OK;
}

extern "C" int kid_pileup_time(kid_pileup *p, double *device_ms, uint64_t *calls, uint64_t *records)
{
    if (!p) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(p->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = kid_pileup_settle(p)) != KID_OK) return rc;
    if (device_ms) *device_ms = p->ms;
    if (calls) *calls = p->calls;
    if (records) *records = p->records;
    p->ms = 0;
    p->calls = p->records = 0;
    return KID_OK;
}
