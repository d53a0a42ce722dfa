// kid_api_shared.h -- k-mers shared between samples: for n seen-bitmaps, per pair and per target, the database entries
// both have a bit for (kernels: kid_shared.hip.h).  Two forms: on a kid_db (its entry -> target map is in HBM already)
// and without one (the caller's targets are uploaded; no table is built).  Neither touches a sample.
#pragma once
#include <mutex>
#include <vector>

#include "kid_shared.hip.h"

// device time of the kernels of the calls so far, for kid_shared_kmers_time (process-wide: the second form has no handle)
static std::mutex g_shared_time_mu;
static double g_shared_time_ms = 0;
static uint64_t g_shared_time_calls = 0;

static int kid_shared_check(const void *const *bitmaps, int n, const int64_t *shared)
{
    if (n < 1 || n > KID_SHARED_MAX_SAMPLES) return kid_fail(KID_ERR_ARG, "n = %d is outside 1..%d", n, KID_SHARED_MAX_SAMPLES);
    if (!bitmaps || !shared) return kid_fail(KID_ERR_ARG, "null argument");
    for (int i = 0; i < n; i++)
        if (!bitmaps[i]) return kid_fail(KID_ERR_ARG, "bitmaps[%d] is null", i);
    return KID_OK;
}

// d_targets: the targets of the entries, padded with zeros to n_words * 32, on the current device
static int kid_shared_run(int num_cu, const uint32_t *d_targets, uint64_t n_entries, uint64_t n_words, int32_t ntar,
                          const void *const *bitmaps, int n, int on_device, int64_t *shared)
{
    const size_t nbytes = (size_t)n_words * 4, total = (size_t)n * n * (size_t)ntar;
    std::vector<const uint32_t *> ptrs((size_t)n);
    KidDevBuf staged, d_ptrs, d_shared;
    if (on_device) {
        for (int i = 0; i < n; i++) {
            if (((uintptr_t)bitmaps[i] & 15u) != 0) return kid_fail(KID_ERR_ARG, "bitmaps[%d]: a bitmap on the device must be 16-byte aligned", i);
            ptrs[(size_t)i] = (const uint32_t *)bitmaps[i];
        }
    } else {
        KID_HIP(staged.alloc(nbytes * (size_t)n));
        for (int i = 0; i < n; i++) {
            KID_HIP(hipMemcpy(staged.as<uint8_t>() + nbytes * (size_t)i, bitmaps[i], nbytes, hipMemcpyHostToDevice));
            ptrs[(size_t)i] = (const uint32_t *)(staged.as<uint8_t>() + nbytes * (size_t)i);
        }
    }
    KID_HIP(d_ptrs.alloc((size_t)n * sizeof(void *)));
    KID_HIP(hipMemcpy(d_ptrs.p, ptrs.data(), (size_t)n * sizeof(void *), hipMemcpyHostToDevice));
    KID_HIP(d_shared.alloc(total * 8));
    KID_HIP(hipMemset(d_shared.p, 0, total * 8));
    const uint64_t n_tiles = (n_entries + KID_SHARED_TILE - 1) / KID_SHARED_TILE;
    KidEvent ev0, ev1;
    KID_HIP(ev0.create());
    KID_HIP(ev1.create());
    KID_HIP(hipDeviceSynchronize()); // (the caller's bitmaps on the device: whatever it queued on other streams is through)
    KID_HIP(hipEventRecord(ev0.e, 0));
    if (n_tiles) {
        // a contiguous span of tiles per workgroup, so that the sums of a target are carried from tile to tile
        uint64_t span = (n_tiles + (uint64_t)num_cu * 8 - 1) / ((uint64_t)num_cu * 8);
        if (span < KID_SHARED_MIN_SPAN) span = KID_SHARED_MIN_SPAN;
        const uint64_t grid = (n_tiles + span - 1) / span;
        const uint32_t npairs = (uint32_t)n * ((uint32_t)n + 1u) / 2u;
        uint32_t split = 1; // few pairs: the lanes share the quads of a pair instead
        while (split < 16u && npairs * split * 2u <= 256u) split *= 2u;
        hipLaunchKernelGGL(kid_shared_kernel, dim3((unsigned)grid), dim3(256), 0, 0, d_ptrs.as<const uint32_t *>(), (uint32_t)n, n_words,
                           d_targets, n_entries, (uint32_t)ntar, n_tiles, span, split, d_shared.as<unsigned long long>());
        if (n > 1)
            hipLaunchKernelGGL(kid_shared_mirror_kernel, dim3(kid_grid_for(total, 256, num_cu * 16)), dim3(256), 0, 0,
                               d_shared.as<unsigned long long>(), (uint32_t)n, (uint32_t)ntar);
        KID_HIP(hipGetLastError());
    }
    KID_HIP(hipEventRecord(ev1.e, 0));
    KID_HIP(hipDeviceSynchronize());
    float ms = 0;
    KID_HIP(hipEventElapsedTime(&ms, ev0.e, ev1.e));
    {
        std::lock_guard<std::mutex> lock(g_shared_time_mu);
        g_shared_time_ms += ms;
        g_shared_time_calls++;
    }
    KID_HIP(hipMemcpy(shared, d_shared.p, total * 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_db_shared_kmers(kid_db *db, const void *const *bitmaps, int n, int on_device, int64_t *shared)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_shared_check(bitmaps, n, shared);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu); // calls on one kid_db run one after the other
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    return kid_shared_run(db->num_cu, db->ord_target.as<uint32_t>(), db->info.n_entries, db->seen_bits / 32, db->info.ntar, bitmaps, n,
                          on_device, shared);
}

extern "C" int kid_shared_kmers(int device, const uint32_t *targets, uint64_t n_entries, int32_t ntar, const void *const *bitmaps, int n,
                                int on_device, int64_t *shared)
{
    int rc = kid_shared_check(bitmaps, n, shared);
    if (rc != KID_OK) return rc;
    if (ntar < 1 || (n_entries && !targets)) return kid_fail(KID_ERR_ARG, "targets is null or ntar < 1");
    if (n_entries >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "more than 2^32-2 entries");
    for (uint64_t o = 0; o < n_entries; o++)
        if (targets[o] >= (uint32_t)ntar) return kid_fail(KID_ERR_TARGET, "targets[%llu] = %u >= ntar", (unsigned long long)o, targets[o]);
    if ((rc = kid_use_device(device)) != KID_OK) return rc;
    int num_cu = 0;
    if (hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || num_cu <= 0) num_cu = 256;
    uint64_t bits = ((n_entries + 127) / 128) * 128; // the padded size a kid_db of n_entries reports
    if (bits == 0) bits = 128;
    KidDevBuf d_targets;
    KID_HIP(d_targets.alloc(bits * 4));
    KID_HIP(hipMemset(d_targets.p, 0, bits * 4));
    if (n_entries) KID_HIP(hipMemcpy(d_targets.p, targets, n_entries * 4, hipMemcpyHostToDevice));
    return kid_shared_run(num_cu, d_targets.as<uint32_t>(), n_entries, bits / 32, ntar, bitmaps, n, on_device, shared);
}

extern "C" int kid_shared_kmers_time(double *device_ms, uint64_t *calls)
{
    std::lock_guard<std::mutex> lock(g_shared_time_mu);
    if (device_ms) *device_ms = g_shared_time_ms;
    if (calls) *calls = g_shared_time_calls;
    g_shared_time_ms = 0;
    g_shared_time_calls = 0;
    return KID_OK;
}
