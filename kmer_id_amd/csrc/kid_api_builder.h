// kid_api_builder.h -- the probe-database builder handle (kmer_build_vf6; kid_build.hip.h).
#pragma once
#include <algorithm>
#include <math.h>
#include <memory>

#include "kid_api_core.h"
#include "kid_build.hip.h"

struct kid_builder {
    int device = 0;
    int32_t ntar = 0;
    uint64_t cell_mask = 0;
    uint64_t batch = 0; // k-mer end positions per chunk
    bool minct_set = false;
    double log10_4 = 0;
    KidStream stream; // (declared first: destroyed last, after the events and buffers used on it)
    KidEvent ev[2];
    // table: 2^log2_cells cells; term: 3 x 20 p*log10(p) of the entropy test; counters: [0] cells filled (0 -> x),
    // [1] candidates of a claim chunk; side_key / side_pos: the claim's side hash (2 slots or more per position)
    KidDevBuf table, parent, minct, term, counters, text, side_key, side_pos, cand;
    double phase_ms[3] = {0, 0, 0}; // device time of add, remove, claim
    uint64_t phase_bases[3] = {0, 0, 0};
};

static_assert(sizeof(KidBuildCand) == sizeof(kid_build_cand), "kid_build_cand layout");

extern "C" int kid_builder_create(int device, int log2_cells, const int32_t *parent, int32_t ntar, uint64_t batch_bases,
                                  kid_builder **out)
{
    if (!out) return kid_fail(KID_ERR_ARG, "out is null");
    *out = nullptr;
    if (!parent || ntar < 2) return kid_fail(KID_ERR_ARG, "parent is null or ntar < 2");
    if (ntar > (1 << 21)) return kid_fail(KID_ERR_ARG, "ntar = %d: targets of 2^21 and more do not fit a cell (target << 11)", ntar);
    if (log2_cells < 10 || log2_cells > 40) return kid_fail(KID_ERR_ARG, "log2_cells = %d outside [10,40]", log2_cells);
    if (batch_bases == 0) batch_bases = (uint64_t)1 << 24;
    if (batch_bases < 64 || batch_bases > ((uint64_t)1 << 30)) return kid_fail(KID_ERR_ARG, "batch_bases outside [64, 2^30]");
    for (int32_t i = 0; i < ntar; i++)
        if (parent[i] < 0 || parent[i] >= ntar) return kid_fail(KID_ERR_TREE, "parent[%d] = %d is outside [0,%d)", i, parent[i], ntar);
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    std::unique_ptr<kid_builder, void (*)(kid_builder *)> b(new kid_builder(), kid_builder_destroy);
    b->device = device;
    b->ntar = ntar;
    b->cell_mask = ((uint64_t)1 << log2_cells) - 1;
    b->batch = batch_bases;
    uint64_t side = 64;
    while (side < 2 * batch_bases) side <<= 1;
    // p*log10(p), p = n / total, exactly as check_entropy computes it (the counts and totals are exact in double)
    double term[60] = {0};
    const int totals[3] = {19, 14, 10};
    for (int f = 0; f < 3; f++)
        for (int n = 1; n <= totals[f]; n++) {
            volatile double p = (double)n / (double)totals[f];
            volatile double l = log10((double)p);
            term[20 * f + n] = p * l;
        }
    b->log10_4 = log10(4.0);
    const uint64_t table_bytes = ((uint64_t)4) << log2_cells;
    KID_HIP(b->stream.create(hipStreamNonBlocking));
    KID_HIP(b->ev[0].create());
    KID_HIP(b->ev[1].create());
    KID_HIP(b->table.alloc(table_bytes));
    KID_HIP(hipMemsetAsync(b->table.p, 0, table_bytes, b->stream.s));
    KID_HIP(b->parent.alloc((size_t)ntar * 4));
    KID_HIP(hipMemcpy(b->parent.p, parent, (size_t)ntar * 4, hipMemcpyHostToDevice));
    KID_HIP(b->minct.alloc((size_t)ntar * 4));
    KID_HIP(b->term.alloc(sizeof(term)));
    KID_HIP(hipMemcpy(b->term.p, term, sizeof(term), hipMemcpyHostToDevice));
    KID_HIP(b->counters.alloc(2 * sizeof(unsigned long long)));
    KID_HIP(hipMemsetAsync(b->counters.p, 0, 2 * sizeof(unsigned long long), b->stream.s));
    KID_HIP(b->text.alloc(batch_bases + 64));
    KID_HIP(b->side_key.alloc(side * sizeof(unsigned long long)));
    KID_HIP(b->side_pos.alloc(side * sizeof(uint32_t)));
    KID_HIP(b->cand.alloc(batch_bases * sizeof(KidBuildCand)));
    KID_HIP(hipStreamSynchronize(b->stream.s));
    *out = b.release();
    return KID_OK;
}

extern "C" void kid_builder_destroy(kid_builder *b)
{
    if (!b) return;
    hipSetDevice(b->device);
    if (b->stream.s) hipStreamSynchronize(b->stream.s);
    delete b;
}

extern "C" int kid_builder_set_minct(kid_builder *b, const int32_t *minct, int32_t n)
{
    if (!b || !minct || n != b->ntar) return kid_fail(KID_ERR_ARG, "null builder / minct, or n != ntar");
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpy(b->minct.p, minct, (size_t)n * 4, hipMemcpyHostToDevice));
    b->minct_set = true;
    return KID_OK;
}

// A text through the device in chunks: k-mer end positions [s, s + batch) with the 29 bases in front.
// launch(first, n, lo) queues a chunk's kernels (text[lo, lo + n), ends from `first` on); done() runs once they are through.
template <class Launch, class Done>
static int kid_builder_chunks(kid_builder *b, const uint8_t *text, uint64_t len, int phase, Launch &&launch, Done &&done)
{
    for (uint64_t s = 0; s < len; s += b->batch) {
        const uint64_t lo = s >= KID_BUILD_K - 1 ? s - (KID_BUILD_K - 1) : 0, hi = std::min(len, s + b->batch);
        KID_HIP(hipMemcpyAsync(b->text.p, text + lo, hi - lo, hipMemcpyHostToDevice, b->stream.s));
        KID_HIP(hipEventRecord(b->ev[0].e, b->stream.s));
        int rc = launch(s - lo, hi - lo, lo);
        if (rc != KID_OK) return rc;
        KID_HIP(hipGetLastError());
        KID_HIP(hipEventRecord(b->ev[1].e, b->stream.s));
        KID_HIP(hipEventSynchronize(b->ev[1].e));
        float ms = 0;
        KID_HIP(hipEventElapsedTime(&ms, b->ev[0].e, b->ev[1].e));
        b->phase_ms[phase] += ms;
        b->phase_bases[phase] += hi - s;
        rc = done();
        if (rc != KID_OK) return rc;
    }
    return KID_OK;
}

static inline dim3 kid_builder_grid(uint64_t first, uint64_t n)
{
    const uint64_t threads = (n - first + KID_BUILD_SEG - 1) / KID_BUILD_SEG;
    return dim3((unsigned)((threads + KID_BUILD_BLOCK - 1) / KID_BUILD_BLOCK));
}

static int kid_builder_nothing() { return KID_OK; }

extern "C" int kid_builder_add(kid_builder *b, const uint8_t *text, uint64_t len, int32_t target)
{
    if (!b || (len && !text)) return kid_fail(KID_ERR_ARG, "null argument");
    if (target >= (1 << 21) || target < 2) return kid_fail(KID_ERR_ARG, "target %d outside [2, 2^21)", target);
    if (target >= b->ntar) return kid_fail(KID_ERR_TARGET, "target %d >= ntar %d", target, b->ntar);
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    return kid_builder_chunks(b, text, len, 0, [&](uint64_t first, uint64_t n, uint64_t) {
        hipLaunchKernelGGL(kid_build_add_kernel, kid_builder_grid(first, n), dim3(KID_BUILD_BLOCK), 0, b->stream.s, b->table.as<uint32_t>(),
                           b->cell_mask, b->text.as<uint8_t>(), first, n, (uint32_t)target, b->parent.as<int32_t>(), b->ntar,
                           b->counters.as<unsigned long long>());
        return KID_OK;
    }, kid_builder_nothing);
}

extern "C" int kid_builder_remove(kid_builder *b, const uint8_t *text, uint64_t len)
{
    if (!b || (len && !text)) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    return kid_builder_chunks(b, text, len, 1, [&](uint64_t first, uint64_t n, uint64_t) {
        hipLaunchKernelGGL(kid_build_remove_kernel, kid_builder_grid(first, n), dim3(KID_BUILD_BLOCK), 0, b->stream.s, b->table.as<uint32_t>(),
                           b->cell_mask, b->text.as<uint8_t>(), first, n);
        return KID_OK;
    }, kid_builder_nothing);
}

extern "C" int kid_builder_claim(kid_builder *b, const uint8_t *text, uint64_t len, int64_t gpos_base, kid_build_cand *out,
                                 uint64_t cap, uint64_t *n_out)
{
    if (!b || !n_out || (len && !text) || (cap && !out)) return kid_fail(KID_ERR_ARG, "null argument");
    if (!b->minct_set) return kid_fail(KID_ERR_STATE, "kid_builder_set_minct has not been called");
    *n_out = 0;
    const uint64_t need = len > KID_BUILD_K - 1 ? len - (KID_BUILD_K - 1) : 0;
    if (cap < need) return kid_fail(KID_ERR_ARG, "cap = %llu < %llu k-mer positions", (unsigned long long)cap, (unsigned long long)need);
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    uint64_t total = 0, ends = 0;
    unsigned long long nc = 0;
    unsigned long long *n_cand = b->counters.as<unsigned long long>() + 1;
    // Chunks one after the other: the first occurrences inside a chunk are the global ones because the chunks (and orgs)
    // in front have already set their cells to 1.
    rc = kid_builder_chunks(b, text, len, 2, [&](uint64_t first, uint64_t n, uint64_t lo) -> int {
        ends = n - first;
        uint64_t side = 64;
        while (side < 2 * ends) side <<= 1;
        KID_HIP(hipMemsetAsync(b->side_key.p, 0, side * sizeof(unsigned long long), b->stream.s));
        KID_HIP(hipMemsetAsync(b->side_pos.p, 0xFF, side * sizeof(uint32_t), b->stream.s));
        KID_HIP(hipMemsetAsync(n_cand, 0, sizeof(unsigned long long), b->stream.s));
        const dim3 grid = kid_builder_grid(first, n);
        const uint8_t *d = b->text.as<uint8_t>();
        hipLaunchKernelGGL(kid_build_claim_kernel, grid, dim3(KID_BUILD_BLOCK), 0, b->stream.s, b->table.as<uint32_t>(), b->cell_mask, d, first, n,
                           b->side_key.as<unsigned long long>(), b->side_pos.as<uint32_t>(), side - 1);
        hipLaunchKernelGGL(kid_build_filter_kernel, grid, dim3(KID_BUILD_BLOCK), 0, b->stream.s, b->table.as<uint32_t>(), b->cell_mask, d, first, n,
                           gpos_base + (int64_t)lo, b->side_key.as<unsigned long long>(), b->side_pos.as<uint32_t>(), side - 1,
                           b->minct.as<int32_t>(), b->term.as<double>(), b->log10_4, b->cand.as<KidBuildCand>(), n_cand, b->batch);
        hipLaunchKernelGGL(kid_build_mark_kernel, grid, dim3(KID_BUILD_BLOCK), 0, b->stream.s, b->table.as<uint32_t>(), b->cell_mask, d, first, n);
        KID_HIP(hipMemcpyAsync(&nc, n_cand, sizeof(nc), hipMemcpyDeviceToHost, b->stream.s));
        return KID_OK;
    }, [&]() -> int {
        if (nc > ends) return kid_fail(KID_ERR_HIP, "a claim chunk gave %llu candidates for %llu positions", nc, (unsigned long long)ends);
        KID_HIP(hipMemcpy(out + total, b->cand.p, nc * sizeof(kid_build_cand), hipMemcpyDeviceToHost));
        std::sort(out + total, out + total + nc, [](const kid_build_cand &x, const kid_build_cand &y) { return x.gpos < y.gpos; });
        total += nc;
        return KID_OK;
    });
    *n_out = total;
    return rc;
}

extern "C" int kid_builder_size(kid_builder *b, uint64_t *n_filled)
{
    if (!b || !n_filled) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    unsigned long long v = 0;
    KID_HIP(hipMemcpy(&v, b->counters.p, sizeof(v), hipMemcpyDeviceToHost));
    *n_filled = v;
    return KID_OK;
}

extern "C" int kid_builder_export(kid_builder *b, uint64_t first_cell, uint64_t n, uint32_t *out)
{
    if (!b || (n && !out)) return kid_fail(KID_ERR_ARG, "null argument");
    if (first_cell > b->cell_mask + 1 || n > b->cell_mask + 1 - first_cell) return kid_fail(KID_ERR_ARG, "cell range outside the table");
    int rc = kid_use_device(b->device);
    if (rc != KID_OK) return rc;
    if (n) KID_HIP(hipMemcpy(out, b->table.as<uint32_t>() + first_cell, n * 4, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_builder_entropy(kid_builder *b, const uint64_t *keys, uint64_t n, uint8_t *flags)
{
    if (!b || (n && (!keys || !flags))) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(b->device);
    if (rc != KID_OK || n == 0) return rc;
    KidDevBuf dk, df;
    KID_HIP(dk.alloc(n * 8));
    KID_HIP(df.alloc(n));
    KID_HIP(hipMemcpy(dk.p, keys, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_build_entropy_kernel, dim3(kid_grid_for(n, 256, 4096)), dim3(256), 0, 0, dk.as<uint64_t>(), n, b->term.as<double>(),
                       b->log10_4, df.as<uint8_t>());
    KID_HIP(hipGetLastError());
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(flags, df.p, n, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_builder_stats(kid_builder *b, double device_ms[3], uint64_t bases[3])
{
    if (!b || !device_ms || !bases) return kid_fail(KID_ERR_ARG, "null argument");
    for (int i = 0; i < 3; i++) {
        device_ms[i] = b->phase_ms[i];
        bases[i] = b->phase_bases[i];
    }
    return KID_OK;
}
