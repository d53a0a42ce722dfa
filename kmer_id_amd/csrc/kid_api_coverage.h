// kid_api_coverage.h -- breadth of coverage per organism from seen-bitmaps and the sites of the entries (kernels:
// kid_coverage.hip.h).  Stateless like kid_shared_kmers: everything is in host memory, no table is built, no sample is
// touched.  The span stage runs once per call; the bitmaps are taken one after the other, each through one upload, one
// clearing of the per-bin counters, the count kernel and the reduce kernel.  Device memory of a call, all of it owned by
// the KidDevBuf members below: 8 bytes per entry (org, pos), one bitmap, 16 bytes per organism (+ 32 per organism for
// the records of the bitmap in flight), and 2 * 4 * B bytes for `probes` and the counters of the bitmap in flight, B being
// at most KID_COVERAGE_MAX_BINS: 2 GiB at the cap.
#pragma once
#include <mutex>
#include <vector>

#include "kid_coverage.hip.h"

static_assert(sizeof(kid_coverage) == sizeof(KidCoverageRec) && sizeof(kid_coverage) == 32, "kid_coverage is the device record");

// device time of the kernels of the calls so far (process-wide: the calls have no handle): all of them, and the count
// kernels over the bitmaps alone
static std::mutex g_coverage_time_mu;
static double g_coverage_time_ms = 0, g_coverage_count_ms = 0;
static uint64_t g_coverage_time_calls = 0;

// out: records [n * n_orgs], or null for the per-bin form, which then writes bin_base / *n_bins and, unless it is the sizing
// call (probes_per_bin null), the two per-bin arrays
static int kid_coverage_run(int device, const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs, uint32_t bin_width,
                            const void *const *bitmaps, int n, kid_coverage *out, uint64_t *bin_base, uint32_t *probes_per_bin,
                            uint32_t *seen_per_bin, uint64_t cap, uint64_t *n_bins)
{
    if (n < 1 || n > KID_SHARED_MAX_SAMPLES) return kid_fail(KID_ERR_ARG, "n = %d is outside 1..%d", n, KID_SHARED_MAX_SAMPLES);
    if (!bitmaps || (n_entries && (!org || !pos))) return kid_fail(KID_ERR_ARG, "null argument");
    for (int i = 0; i < n; i++)
        if (!bitmaps[i]) return kid_fail(KID_ERR_ARG, "bitmaps[%d] is null", i);
    if (bin_width == 0) return kid_fail(KID_ERR_ARG, "bin_width is 0");
    if (n_entries >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "more than 2^32-2 entries");
    for (uint64_t o = 0; o < n_entries; o++)
        if (org[o] >= n_orgs) return kid_fail(KID_ERR_ARG, "org[%llu] = %u >= n_orgs = %u", (unsigned long long)o, org[o], n_orgs);
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    int num_cu = 0;
    if (hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || num_cu <= 0) num_cu = 256;
    uint64_t bits = ((n_entries + 127) / 128) * 128; // the padded size a kid_db of n_entries reports
    if (bits == 0) bits = 128;
    const size_t map_bytes = (size_t)(bits / 8);

    KidDevBuf d_org, d_pos, d_span, d_base, d_map, d_probes, d_seen, d_recs;
    std::vector<KidEvent> marks; // [0] .. [1]: the span stage; then per stage of the rest its first and last
    auto mark = [&]() -> hipError_t {
        marks.emplace_back();
        hipError_t e = marks.back().create();
        return e != hipSuccess ? e : hipEventRecord(marks.back().e, 0);
    };
    KID_HIP(d_org.alloc((size_t)n_entries * 4));
    KID_HIP(d_pos.alloc((size_t)n_entries * 4));
    if (n_entries) {
        KID_HIP(hipMemcpy(d_org.p, org, (size_t)n_entries * 4, hipMemcpyHostToDevice));
        KID_HIP(hipMemcpy(d_pos.p, pos, (size_t)n_entries * 4, hipMemcpyHostToDevice));
    }
    KID_HIP(d_span.alloc((size_t)n_orgs * 4));
    KID_HIP(d_base.alloc(((size_t)n_orgs + 1) * 8));
    KID_HIP(hipMemset(d_span.p, 0, d_span.cap));
    KID_HIP(hipDeviceSynchronize());
    // ---- span: span_bins per organism, bin_base, B
    KID_HIP(mark());
    if (n_entries)
        hipLaunchKernelGGL(kid_cov_span_kernel, dim3(kid_grid_for(n_entries, 256, num_cu * 8)), dim3(256), 0, 0, d_org.as<uint32_t>(),
                           d_pos.as<uint32_t>(), n_entries, n_orgs, bin_width, d_span.as<uint32_t>());
    hipLaunchKernelGGL(kid_cov_scan_kernel, dim3(1), dim3(256), 0, 0, d_span.as<uint32_t>(), n_orgs, d_base.as<unsigned long long>());
    KID_HIP(hipGetLastError());
    KID_HIP(mark());
    uint64_t B = 0;
    KID_HIP(hipMemcpy(&B, d_base.as<unsigned long long>() + n_orgs, 8, hipMemcpyDeviceToHost));
    if (B > KID_COVERAGE_MAX_BINS)
        return kid_fail(KID_ERR_ARG, "%llu bins of %u bases over all organisms: more than KID_COVERAGE_MAX_BINS", (unsigned long long)B, bin_width);
    const bool sizing = !out && !probes_per_bin;
    if (!out && !sizing && cap < B) return kid_fail(KID_ERR_ARG, "room for %llu bins where there are %llu", (unsigned long long)cap, (unsigned long long)B);
    std::vector<size_t> count_marks; // the marks in front of the count kernels over the bitmaps
    if (!sizing) {
        const uint64_t n_tiles = (n_entries + KID_COV_TILE - 1) / KID_COV_TILE;
        // a contiguous span of tiles per workgroup: the atomics of a bin come from few workgroups
        uint64_t span = (n_tiles + (uint64_t)num_cu * 16 - 1) / ((uint64_t)num_cu * 16);
        if (span < KID_COV_MIN_SPAN) span = KID_COV_MIN_SPAN;
        const unsigned grid = (unsigned)((n_tiles + span - 1) / span);
        KID_HIP(d_probes.alloc((size_t)B * 4));
        KID_HIP(d_seen.alloc((size_t)B * 4));
        KID_HIP(d_map.alloc(map_bytes));
        if (out) KID_HIP(d_recs.alloc((size_t)n_orgs * sizeof(KidCoverageRec)));
        // ---- probes per bin: the count kernel over every entry
        KID_HIP(hipMemset(d_probes.p, 0, d_probes.cap));
        KID_HIP(hipDeviceSynchronize());
        KID_HIP(mark());
        if (n_tiles)
            hipLaunchKernelGGL(kid_cov_count_kernel<true>, dim3(grid), dim3(256), 0, 0, (const unsigned long long *)nullptr, d_org.as<uint32_t>(),
                               d_pos.as<uint32_t>(), n_entries, n_orgs, bin_width, d_base.as<unsigned long long>(), B, n_tiles, span,
                               d_probes.as<uint32_t>());
        KID_HIP(hipGetLastError());
        KID_HIP(mark());
        // ---- the bitmaps, one after the other
        for (int i = 0; i < n; i++) {
            KID_HIP(hipMemcpy(d_map.p, bitmaps[i], map_bytes, hipMemcpyHostToDevice));
            KID_HIP(hipMemset(d_seen.p, 0, d_seen.cap));
            KID_HIP(hipDeviceSynchronize());
            count_marks.push_back(marks.size());
            KID_HIP(mark());
            if (n_tiles)
                hipLaunchKernelGGL(kid_cov_count_kernel<false>, dim3(grid), dim3(256), 0, 0, d_map.as<unsigned long long>(), d_org.as<uint32_t>(),
                                   d_pos.as<uint32_t>(), n_entries, n_orgs, bin_width, d_base.as<unsigned long long>(), B, n_tiles, span,
                                   d_seen.as<uint32_t>());
            KID_HIP(hipGetLastError());
            KID_HIP(mark());
            if (out) {
                KID_HIP(mark());
                if (n_orgs)
                    hipLaunchKernelGGL(kid_cov_reduce_kernel, dim3(kid_grid_for((uint64_t)n_orgs * 64, 256, num_cu * 16)), dim3(256), 0, 0,
                                       d_span.as<uint32_t>(), d_base.as<unsigned long long>(), d_probes.as<uint32_t>(), d_seen.as<uint32_t>(),
                                       n_orgs, d_recs.as<KidCoverageRec>());
                KID_HIP(hipGetLastError());
                KID_HIP(mark());
                if (n_orgs) KID_HIP(hipMemcpy(out + (size_t)i * n_orgs, d_recs.p, (size_t)n_orgs * sizeof(KidCoverageRec), hipMemcpyDeviceToHost));
            } else if (B) {
                KID_HIP(hipMemcpy(seen_per_bin + (size_t)i * B, d_seen.p, (size_t)B * 4, hipMemcpyDeviceToHost));
            }
        }
        if (!out && B) KID_HIP(hipMemcpy(probes_per_bin, d_probes.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    }
    if (!out) {
        KID_HIP(hipMemcpy(bin_base, d_base.p, ((size_t)n_orgs + 1) * 8, hipMemcpyDeviceToHost));
        *n_bins = B;
    }
    KID_HIP(hipDeviceSynchronize());
    double all_ms = 0, count_ms = 0;
    for (size_t m = 0; m + 1 < marks.size(); m += 2) {
        float ms = 0;
        KID_HIP(hipEventElapsedTime(&ms, marks[m].e, marks[m + 1].e));
        all_ms += ms;
        for (size_t c : count_marks)
            if (c == m) count_ms += ms;
    }
    {
        std::lock_guard<std::mutex> lock(g_coverage_time_mu);
        g_coverage_time_ms += all_ms;
        g_coverage_count_ms += count_ms;
        g_coverage_time_calls++;
    }
    return KID_OK;
}

extern "C" int kid_seen_coverage(int device, const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs,
                                 uint32_t bin_width, const void *const *bitmaps, int n, kid_coverage *out)
{
    if (!out) return kid_fail(KID_ERR_ARG, "null argument");
    return kid_coverage_run(device, org, pos, n_entries, n_orgs, bin_width, bitmaps, n, out, nullptr, nullptr, nullptr, 0, nullptr);
}

extern "C" int kid_seen_coverage_bins(int device, const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs,
                                      uint32_t bin_width, const void *const *bitmaps, int n, uint64_t *bin_base, uint32_t *probes_per_bin,
                                      uint32_t *seen_per_bin, uint64_t cap, uint64_t *n_bins)
{
    if (!bin_base || !n_bins) return kid_fail(KID_ERR_ARG, "null argument");
    // both arrays, or neither and no room: the sizing call
    if ((probes_per_bin == nullptr) != (seen_per_bin == nullptr) || (!probes_per_bin && cap != 0))
        return kid_fail(KID_ERR_ARG, "probes_per_bin and seen_per_bin go together, and without them cap is 0");
    return kid_coverage_run(device, org, pos, n_entries, n_orgs, bin_width, bitmaps, n, nullptr, bin_base, probes_per_bin, seen_per_bin, cap,
                            n_bins);
}

extern "C" int kid_seen_coverage_time(double *device_ms, uint64_t *calls)
{
    std::lock_guard<std::mutex> lock(g_coverage_time_mu);
    if (device_ms) *device_ms = g_coverage_time_ms;
    if (calls) *calls = g_coverage_time_calls;
    g_coverage_time_ms = 0;
    g_coverage_time_calls = 0;
    return KID_OK;
}

extern "C" int kid_bench_coverage_count_time(double *count_ms)
{
    std::lock_guard<std::mutex> lock(g_coverage_time_mu);
    if (count_ms) *count_ms = g_coverage_count_ms;
    g_coverage_count_ms = 0;
    return KID_OK;
}
