// kid_api_depth.h -- k-mer depth per database entry: the sample option KID_OPT_ENTRY_DEPTH, the export / add pair of the
// counter array and the per-target depth spectrum, of one sample or of several samples' sum (kernels: kid_depth.hip.h).
// The counters themselves are added to by the tally of kid_api_support.h.  Included behind the sample handle.
#pragma once
#include "kid_depth.hip.h"

static inline uint64_t kid_depth_words(const kid_sample *s) { return s->seen_words * 32; } // the entries, padded to 128

// KID_OPT_ENTRY_DEPTH: 1 allocates the counters (zeroed; a no-op while they exist), 0 frees them
static int kid_depth_set_option(kid_sample *s, int value)
{
    if (value != 0 && value != 1) return kid_fail(KID_ERR_ARG, "KID_OPT_ENTRY_DEPTH: the value is 0 or 1, not %d", value);
    if ((value == 1) == (s->depth.p != nullptr)) return KID_OK;
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize()); // a tally may still be adding
    if (value == 0) {
        s->depth.reset();
        return KID_OK;
    }
    KidDevBuf buf;
    KID_HIP(buf.alloc(kid_depth_words(s) * 4));
    KID_HIP(hipMemset(buf.p, 0, kid_depth_words(s) * 4));
    s->depth = std::move(buf);
    return KID_OK;
}

// the sample's counters, at rest: the option is on and everything queued on the sample's device is through
static int kid_depth_at_rest(kid_sample *s)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    if (!s->depth.p) return kid_fail(KID_ERR_STATE, "KID_OPT_ENTRY_DEPTH is off for this sample");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

static int kid_depth_check_range(const kid_sample *s, uint64_t entry_begin, uint64_t n, const void *p)
{
    const uint64_t ne = s->db->info.n_entries;
    if (entry_begin > ne || n > ne - entry_begin)
        return kid_fail(KID_ERR_ARG, "entries [%llu, +%llu) lie outside the %llu entries of the database", (unsigned long long)entry_begin,
                        (unsigned long long)n, (unsigned long long)ne);
    if (n && !p) return kid_fail(KID_ERR_ARG, "null argument");
    return KID_OK;
}

extern "C" int kid_sample_depth_export(kid_sample *s, uint64_t entry_begin, uint64_t n, void *dst, int dst_on_device)
{
    int rc = kid_depth_at_rest(s);
    if (rc != KID_OK) return rc;
    if ((rc = kid_depth_check_range(s, entry_begin, n, dst)) != KID_OK) return rc;
    if (n) KID_HIP(hipMemcpy(dst, s->depth.as<uint32_t>() + entry_begin, n * 4, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_depth_add(kid_sample *s, uint64_t entry_begin, uint64_t n, const void *src, int src_on_device)
{
    int rc = kid_depth_at_rest(s);
    if (rc != KID_OK) return rc;
    if ((rc = kid_depth_check_range(s, entry_begin, n, src)) != KID_OK) return rc;
    if (n == 0) return KID_OK;
    const uint32_t *dsrc = (const uint32_t *)src;
    KidDevBuf tmp;
    if (!src_on_device) {
        KID_HIP(tmp.alloc(n * 4));
        KID_HIP(hipMemcpy(tmp.p, src, n * 4, hipMemcpyHostToDevice));
        dsrc = tmp.as<uint32_t>();
    }
    hipLaunchKernelGGL(kid_depth_add_kernel, dim3(kid_grid_for(n, 256, s->db->num_cu * 16)), dim3(256), 0, 0, s->depth.as<uint32_t>() + entry_begin,
                       dsrc, n);
    KID_HIP(hipGetLastError());
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

// entries per target of the database, made by the first spectrum that asks (the current device is db's)
static int kid_depth_entries_per_target(kid_db *db, const unsigned long long **out)
{
    std::lock_guard<std::mutex> lock(db->hits_mu);
    if (!db->entries_per_target.p) {
        const size_t nt = (size_t)db->info.ntar;
        KidDevBuf buf;
        KID_HIP(buf.alloc(nt * 8));
        KID_HIP(hipMemset(buf.p, 0, nt * 8));
        if (db->info.n_entries) {
            hipLaunchKernelGGL(kid_depth_entries_kernel, dim3(kid_grid_for(db->info.n_entries, 256, db->num_cu * 8)), dim3(256), 0, 0,
                               db->ord_target.as<uint32_t>(), db->info.n_entries, (uint32_t)nt, buf.as<unsigned long long>());
            KID_HIP(hipGetLastError());
        }
        KID_HIP(hipDeviceSynchronize());
        db->entries_per_target = std::move(buf);
    }
    *out = db->entries_per_target.as<unsigned long long>();
    return KID_OK;
}

static int kid_depth_check_bins(uint32_t bins)
{
    if (bins < 2u || bins > KID_DEPTH_MAX_BINS) return kid_fail(KID_ERR_ARG, "bins = %u is outside 2..%u", bins, KID_DEPTH_MAX_BINS);
    return KID_OK;
}

// the spectrum of `d_depth` (counters numbered like db's entries, at rest on db's device, which is current)
static int kid_depth_spectrum_of(kid_db *db, const uint32_t *d_depth, uint64_t words, uint32_t bins, uint64_t *spectrum, uint64_t *ksum,
                                 uint32_t *dmax)
{
    const unsigned long long *per_target = nullptr;
    int rc = kid_depth_entries_per_target(db, &per_target);
    if (rc != KID_OK) return rc;
    const size_t nt = (size_t)db->info.ntar;
    const uint32_t ntar = (uint32_t)nt;
    KidDevBuf d_spec, d_ksum, d_dmax;
    KID_HIP(d_spec.alloc(nt * bins * 8));
    KID_HIP(d_ksum.alloc(nt * 8));
    KID_HIP(d_dmax.alloc(nt * 4));
    KID_HIP(hipMemset(d_spec.p, 0, nt * bins * 8));
    KID_HIP(hipMemset(d_ksum.p, 0, nt * 8));
    KID_HIP(hipMemset(d_dmax.p, 0, nt * 4));
    const uint64_t n_quads = words / 4;
    hipLaunchKernelGGL(kid_depth_spectrum_kernel, dim3(kid_grid_for(n_quads, 256, db->num_cu * 8)), dim3(256), 0, 0, d_depth, n_quads,
                       db->ord_target.as<uint32_t>(), ntar, bins, d_spec.as<unsigned long long>(), d_ksum.as<unsigned long long>(),
                       d_dmax.as<uint32_t>());
    hipLaunchKernelGGL(kid_depth_column0_kernel, dim3(kid_grid_for(nt, 4, db->num_cu * 8)), dim3(256), 0, 0, d_spec.as<unsigned long long>(),
                       per_target, ntar, bins);
    KID_HIP(hipGetLastError());
    KID_HIP(hipDeviceSynchronize());
    if (spectrum) KID_HIP(hipMemcpy(spectrum, d_spec.p, nt * bins * 8, hipMemcpyDeviceToHost));
    if (ksum) KID_HIP(hipMemcpy(ksum, d_ksum.p, nt * 8, hipMemcpyDeviceToHost));
    if (dmax) KID_HIP(hipMemcpy(dmax, d_dmax.p, nt * 4, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_depth_spectrum(kid_sample *s, uint32_t bins, uint64_t *spectrum, uint64_t *ksum, uint32_t *dmax)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    int rc = kid_depth_check_bins(bins);
    if (rc != KID_OK) return rc;
    if ((rc = kid_depth_at_rest(s)) != KID_OK) return rc;
    return kid_depth_spectrum_of(s->db, s->depth.as<uint32_t>(), kid_depth_words(s), bins, spectrum, ksum, dmax);
}

// One input sample dealt over n kid_sample objects on replicas: the counter arrays are summed, with saturation, into
// scratch on samples[0]'s device (peer copies, as kid_sample_end_merged moves the bitmaps), and the spectrum is that of
// the sum.  No sample's counters change.
extern "C" int kid_sample_depth_spectrum_merged(kid_sample **samples, int n, uint32_t bins, uint64_t *spectrum, uint64_t *ksum, uint32_t *dmax)
{
    if (!samples || n < 1) return kid_fail(KID_ERR_ARG, "bad argument");
    int rc = kid_depth_check_bins(bins);
    if (rc != KID_OK) return rc;
    for (int i = 0; i < n; i++) {
        if (!samples[i]) return kid_fail(KID_ERR_ARG, "samples[%d] is null", i);
        if (samples[i]->seen_words != samples[0]->seen_words || samples[i]->db->info.ntar != samples[0]->db->info.ntar ||
            samples[i]->db->info.n_entries != samples[0]->db->info.n_entries)
            return kid_fail(KID_ERR_ARG, "samples[%d] belongs to a database built from other entries", i);
        for (int j = 0; j < i; j++)
            if (samples[i] == samples[j]) return kid_fail(KID_ERR_ARG, "samples[%d] and samples[%d] are the same sample (its hits would be counted twice)", j, i);
    }
    for (int i = 0; i < n; i++)
        if (!samples[i]->depth.p) return kid_fail(KID_ERR_STATE, "KID_OPT_ENTRY_DEPTH is off for samples[%d]", i);
    kid_sample *s0 = samples[0];
    if (n == 1) return kid_sample_depth_spectrum(s0, bins, spectrum, ksum, dmax);
    for (int i = 1; i < n; i++) // the others' devices: nothing is adding to their counters any more
        if ((rc = kid_depth_at_rest(samples[i])) != KID_OK) return rc;
    if ((rc = kid_depth_at_rest(s0)) != KID_OK) return rc;
    const uint64_t words = kid_depth_words(s0);
    const size_t nbytes = (size_t)words * 4;
    KidDevBuf sum, tmp;
    KID_HIP(sum.alloc(nbytes));
    KID_HIP(tmp.alloc(nbytes));
    KID_HIP(hipMemcpy(sum.p, s0->depth.p, nbytes, hipMemcpyDeviceToDevice));
    for (int i = 1; i < n; i++) {
        if (samples[i]->db->device == s0->db->device) KID_HIP(hipMemcpy(tmp.p, samples[i]->depth.p, nbytes, hipMemcpyDeviceToDevice));
        else KID_HIP(hipMemcpyPeer(tmp.p, s0->db->device, samples[i]->depth.p, samples[i]->db->device, nbytes));
        hipLaunchKernelGGL(kid_depth_add_kernel, dim3(kid_grid_for(words, 256, s0->db->num_cu * 16)), dim3(256), 0, 0, sum.as<uint32_t>(),
                           tmp.as<uint32_t>(), words);
        KID_HIP(hipGetLastError());
        KID_HIP(hipDeviceSynchronize());
    }
    return kid_depth_spectrum_of(s0->db, sum.as<uint32_t>(), words, bins, spectrum, ksum, dmax);
}
