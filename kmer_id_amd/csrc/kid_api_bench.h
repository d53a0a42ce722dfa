// kid_api_bench.h -- what benchmarks, tools and front-ends need beside classification: the synthetic workload, the
// gather micro-benchmark, raw device memory (include/kmer_id_amd_bench.h), the device's memory figures and page-locked
// host memory.  kid_dev_free and kid_host_free give back memory the CALLER holds: no owner type fits a raw pointer
// that crosses the C ABI, and they report the runtime's status.
#pragma once
#include <ctype.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include "kid_api_db.h"
#include "kid_bench.hip.h"

// ---------------------------------------------------------------- synthetic workload
extern "C" int kid_synth_db_keys_host(uint64_t seed, int k, const uint64_t *cum, int32_t ntar, uint64_t j0, uint64_t n,
                                      uint64_t *keys, uint32_t *targets)
{
    if (!cum || !keys || !targets || ntar < 1 || k < 1 || k > 31) return kid_fail(KID_ERR_ARG, "bad argument");
    for (uint64_t i = 0; i < n; i++) {
        keys[i] = kid_synth_db_key(seed, k, j0 + i);
        targets[i] = kid_synth_target_of(cum, ntar, j0 + i);
    }
    return KID_OK;
}

extern "C" int kid_synth_db_keys_device(uint64_t seed, int k, const uint64_t *cum_host, int32_t ntar, uint64_t j0, uint64_t n,
                                        void *d_keys, void *d_targets, int device)
{
    if (!cum_host || !d_keys || !d_targets || ntar < 1 || k < 1 || k > 31) return kid_fail(KID_ERR_ARG, "bad argument");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    KidDevBuf dcum;
    KID_HIP(dcum.alloc(((size_t)ntar + 1) * 8));
    KID_HIP(hipMemcpy(dcum.p, cum_host, ((size_t)ntar + 1) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_synth_keys_kernel, dim3(kid_grid_for(n, 256, 256 * 16)), dim3(256), 0, 0, seed, k, dcum.as<uint64_t>(),
                       ntar, j0, n, (uint64_t *)d_keys, (uint32_t *)d_targets);
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

extern "C" int kid_synth_reads_host(uint64_t db_seed, uint64_t read_seed, int k, const uint64_t *cum, const int32_t *parent,
                                    int32_t ntar, uint64_t r0, uint64_t n_reads, uint32_t read_len, uint8_t *bases)
{
    if (!cum || !parent || !bases || ntar < 2 || k < 1 || k > 31 || read_len == 0) return kid_fail(KID_ERR_ARG, "bad argument");
    for (uint64_t i = 0; i < n_reads; i++)
        kid_synth_read(db_seed, read_seed, k, cum, parent, ntar, r0 + i, read_len, bases + i * (uint64_t)read_len);
    return KID_OK;
}

extern "C" int kid_synth_reads_device(uint64_t db_seed, uint64_t read_seed, int k, const uint64_t *cum_host,
                                      const int32_t *parent_host, int32_t ntar, uint64_t r0, uint64_t n_reads,
                                      uint32_t read_len, void *d_bases, int device)
{
    if (!cum_host || !parent_host || !d_bases || ntar < 2 || k < 1 || k > 31 || read_len == 0)
        return kid_fail(KID_ERR_ARG, "bad argument");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    KidDevBuf dcum, dpar;
    KID_HIP(dcum.alloc(((size_t)ntar + 1) * 8));
    KID_HIP(dpar.alloc((size_t)ntar * 4));
    KID_HIP(hipMemcpy(dcum.p, cum_host, ((size_t)ntar + 1) * 8, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(dpar.p, parent_host, (size_t)ntar * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_synth_reads_kernel, dim3(kid_grid_for(n_reads, 256, 256 * 16)), dim3(256), 0, 0, db_seed, read_seed, k,
                       dcum.as<uint64_t>(), dpar.as<int32_t>(), ntar, r0, n_reads, read_len, (uint8_t *)d_bases);
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

extern "C" int kid_bench_gather(kid_db *db, uint64_t n_loads, int inflight, int iters, float *ms_out, uint64_t *loads_out)
{
    if (!db || !ms_out || !loads_out || iters < 1) return kid_fail(KID_ERR_ARG, "bad argument");
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    const int block = 256, grid = db->num_cu * 8;
    const uint64_t lanes = (uint64_t)block * grid;
    // inflight = 101 / 108: random LINES, runs of 1 / 8 lanes on a line, 4 loads in flight (kid_gather_lines_kernel);
    // *loads_out is then the number of distinct line requests
    // inflight = 201 / 208: the same two shapes on the digest plane (8-byte loads; a table without one: KID_ERR_ARG)
    const bool by_digest = inflight == 201 || inflight == 208;
    const bool by_line = by_digest || inflight == 101 || inflight == 108 || inflight == 111 || inflight == 121 || inflight == 131; // (1x1: development variants, see the kernel)
    if (!by_line && inflight != 1 && inflight != 2 && inflight != 4 && inflight != 8) return kid_fail(KID_ERR_ARG, "inflight must be 1,2,4 or 8 (or 101, 108: by line)");
    if (by_line && db->d.slot_mask < 7u) return kid_fail(KID_ERR_ARG, "table too small");
    if (by_digest && !db->d.digest) return kid_fail(KID_ERR_ARG, "the table has no digest plane");
    uint64_t rounds = n_loads / (lanes * (uint64_t)(by_line ? 4 : inflight));
    if (rounds < 1) rounds = 1;
    KidDevBuf sinkb;
    KID_HIP(sinkb.alloc(16));
    uint32_t *const sink = sinkb.as<uint32_t>();
    KidEvent ev0, ev1;
    KID_HIP(ev0.create());
    KID_HIP(ev1.create());
    const hipEvent_t e0 = ev0.e, e1 = ev1.e;
    auto launch = [&]() {
        const uint32_t line_mask = db->d.slot_mask >> 3;
        switch (inflight) {
        case 101: hipLaunchKernelGGL((kid_gather_lines_kernel<1>), dim3(grid), dim3(block), 0, 0, db->d.table, line_mask, rounds, sink); break;
        case 111: hipLaunchKernelGGL((kid_gather_lines_kernel<1, 1>), dim3(grid), dim3(block), 0, 0, db->d.table, line_mask, rounds, sink); break;
        case 121: hipLaunchKernelGGL((kid_gather_lines_kernel<1, 2>), dim3(grid), dim3(block), 0, 0, db->d.table, line_mask, rounds, sink); break;
        case 131: hipLaunchKernelGGL((kid_gather_lines_kernel<1, 3>), dim3(grid), dim3(block), 0, 0, db->d.table, line_mask, rounds, sink); break;
        case 108: hipLaunchKernelGGL((kid_gather_lines_kernel<8>), dim3(grid), dim3(block), 0, 0, db->d.table, line_mask, rounds, sink); break;
        case 201: hipLaunchKernelGGL((kid_gather_digest_kernel<1>), dim3(grid), dim3(block), 0, 0, db->d.digest, line_mask, rounds, sink); break;
        case 208: hipLaunchKernelGGL((kid_gather_digest_kernel<8>), dim3(grid), dim3(block), 0, 0, db->d.digest, line_mask, rounds, sink); break;
        case 1: hipLaunchKernelGGL((kid_gather_kernel<1>), dim3(grid), dim3(block), 0, 0, db->d.table, db->d.slot_mask, rounds, sink); break;
        case 2: hipLaunchKernelGGL((kid_gather_kernel<2>), dim3(grid), dim3(block), 0, 0, db->d.table, db->d.slot_mask, rounds, sink); break;
        case 4: hipLaunchKernelGGL((kid_gather_kernel<4>), dim3(grid), dim3(block), 0, 0, db->d.table, db->d.slot_mask, rounds, sink); break;
        default: hipLaunchKernelGGL((kid_gather_kernel<8>), dim3(grid), dim3(block), 0, 0, db->d.table, db->d.slot_mask, rounds, sink); break;
        }
    };
    launch(); // warm-up
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; i++) launch();
    KID_HIP(hipEventRecord(e1, 0));
    KID_HIP(hipEventSynchronize(e1));
    float ms = 0;
    KID_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / (float)iters;
    *loads_out = by_line ? rounds * (lanes / (inflight == 108 || inflight == 208 ? 8 : 1)) * 4 : rounds * lanes * (uint64_t)inflight; // loads (lines) actually asked for per launch
    return KID_OK;
}

// where the table and its digest plane lie in device memory (kid_dev_download reads them): for tests and tools
extern "C" int kid_bench_db_arrays(struct kid_db *db, const void **table, uint64_t *table_bytes, const void **digest, uint64_t *digest_bytes)
{
    if (!db || !table || !table_bytes || !digest || !digest_bytes) return kid_fail(KID_ERR_ARG, "null argument");
    *table = db->table.p;
    *table_bytes = db->info.table_bytes;
    *digest = db->digest.p;
    *digest_bytes = db->digest.p ? db->info.table_bytes / 16 : 0;
    return KID_OK;
}

// ---------------------------------------------------------------- device memory helpers
extern "C" int kid_dev_alloc(int device, uint64_t nbytes, void **d_ptr)
{
    if (!d_ptr) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMalloc(d_ptr, nbytes ? nbytes : 16));
    return KID_OK;
}
extern "C" int kid_dev_free(int device, void *d_ptr)
{
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    if (d_ptr) KID_HIP(hipFree(d_ptr));
    return KID_OK;
}
extern "C" int kid_dev_upload(int device, void *d_dst, const void *src, uint64_t nbytes)
{
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    if (nbytes) KID_HIP(hipMemcpy(d_dst, src, nbytes, hipMemcpyHostToDevice));
    return KID_OK;
}
extern "C" int kid_dev_download(int device, void *dst, const void *d_src, uint64_t nbytes)
{
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    if (nbytes) KID_HIP(hipMemcpy(dst, d_src, nbytes, hipMemcpyDeviceToHost));
    return KID_OK;
}
extern "C" int kid_dev_sync(int device)
{
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

extern "C" int kid_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes)
{
    if (!free_bytes || !total_bytes) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    size_t f = 0, t = 0;
    KID_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = f;
    *total_bytes = t;
    return KID_OK;
}

// ---------------------------------------------------------------- page-locked host memory

// CPUs of the NUMA node the GPU's PCIe root port hangs off (sysfs); false when the box does not say
static bool kid_device_local_cpus(int device, cpu_set_t *set)
{
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) return false;
    for (char *c = bdf; *c; c++) *c = (char)tolower(*c);
    char path[256];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    if (node < 0) return false;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return false;
    char list[4096] = {0};
    const bool ok = fgets(list, sizeof(list), f) != nullptr;
    fclose(f);
    if (!ok) return false;
    CPU_ZERO(set);
    int n = 0;
    for (char *p = list; *p;) { // "0-63,128-191"
        char *end;
        long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) { CPU_SET((int)c, set); n++; }
        p = (*end == ',') ? end + 1 : end;
        if (*end != ',' ) break;
    }
    return n > 0;
}

extern "C" int kid_host_alloc(int device, uint64_t nbytes, void **ptr)
{
    if (!ptr) return kid_fail(KID_ERR_ARG, "null argument");
    *ptr = nullptr;
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    // Page-locked memory is placed where the allocating thread runs; DMA from the other socket's memory reaches the
    // GPU at little more than half the PCIe rate (measured 32 vs 55 GB/s).  So: allocate from a CPU next to the GPU.
    cpu_set_t old_set, local;
    const bool have_old = sched_getaffinity(0, sizeof(old_set), &old_set) == 0;
    bool moved = false;
    if (have_old && kid_device_local_cpus(device, &local)) {
        cpu_set_t both;
        CPU_AND(&both, &local, &old_set); // never leave the CPUs this process was given
        if (CPU_COUNT(&both) > 0) moved = sched_setaffinity(0, sizeof(both), &both) == 0;
    }
    hipError_t e = hipHostMalloc(ptr, nbytes ? nbytes : 16, hipHostMallocDefault);
    if (moved) sched_setaffinity(0, sizeof(old_set), &old_set);
    if (e != hipSuccess) {
        *ptr = nullptr;
        return kid_fail(e == hipErrorOutOfMemory ? KID_ERR_NOMEM : KID_ERR_HIP, "hipHostMalloc(%llu) failed: %s",
                        (unsigned long long)nbytes, hipGetErrorString(e));
    }
    return KID_OK;
}

extern "C" int kid_host_free(void *ptr)
{
    if (ptr) KID_HIP(hipHostFree(ptr));
    return KID_OK;
}
