// kid_api_lowc.h -- mask low-complexity sequence (kid_lowc.hip.h): the range check of T, the launch (one kernel in
// place while no line is split, else plane + mark + apply), and kid_lowc_batch / kid_lowc_batch_device.  The database's
// option is set in kid_db_set_option (kid_api_mask.h) and used by kid_hits_stage_fastq; the sample's option and counter
// are with the sample (kid_api.hip).
#pragma once
#include "kid_api_db.h"
#include "kid_lowc.hip.h"

#define KID_MAX_LOW_COMPLEXITY 1000

static int kid_lowc_check_t(int t)
{
    if (t < 0 || t > KID_MAX_LOW_COMPLEXITY) return kid_fail(KID_ERR_ARG, "low_complexity = %d outside [0, %d]", t, KID_MAX_LOW_COMPLEXITY);
    return KID_OK;
}

// Text in HBM, t > 0, n > 0, on `stream`.  The lines: d_recs (a FASTQ block's records), else d_offsets[0 .. n].
// longest: the longest line where the host knows it -- a line longer than KID_LOWC_CHUNK is split among lanes, and the
// batch then takes the two passes through `plane` (grown here to text_nbytes: the caller sees to it that nothing uses
// it any more) -- or 0: the lines are not split (and neither plane nor text_nbytes is used).
static int kid_lowc_launch(const kid_db *db, uint8_t *d_text, uint64_t text_nbytes, const KidFastqRec *d_recs, const uint64_t *d_offsets,
                           uint64_t n, uint64_t longest, int t, KidDevBuf *plane, unsigned long long *d_n_masked, hipStream_t stream)
{
    const uint32_t base_bits = KID_LOWC_BASE_BITS(db->d.u_is_t);
    if (longest <= KID_LOWC_CHUNK) {
        const dim3 grid(kid_grid_for(n, KID_LOWC_BLOCK, db->num_cu * 16));
        if (d_recs)
            hipLaunchKernelGGL((kid_lowc_mark_kernel<true, false>), grid, dim3(KID_LOWC_BLOCK), 0, stream, d_text, d_recs,
                               (const uint64_t *)nullptr, n, 1u, (uint32_t)t, base_bits, (uint8_t *)nullptr, d_n_masked);
        else
            hipLaunchKernelGGL((kid_lowc_mark_kernel<false, false>), grid, dim3(KID_LOWC_BLOCK), 0, stream, d_text, (const KidFastqRec *)nullptr,
                               d_offsets, n, 1u, (uint32_t)t, base_bits, (uint8_t *)nullptr, d_n_masked);
        KID_HIP(hipGetLastError());
        return KID_OK;
    }
    uint64_t parts = (longest + KID_LOWC_CHUNK - 1) / KID_LOWC_CHUNK;
    if (parts > KID_LOWC_MAX_PARTS) parts = KID_LOWC_MAX_PARTS;
    const uint64_t plane_bytes = (text_nbytes + 15) & ~15ull;
    KID_HIP(plane->ensure(plane_bytes, plane_bytes + plane_bytes / 8));
    KID_HIP(hipMemsetAsync(plane->p, 0, plane_bytes, stream));
    const dim3 grid(kid_grid_for(n * parts, KID_LOWC_BLOCK, db->num_cu * 16));
    if (d_recs)
        hipLaunchKernelGGL((kid_lowc_mark_kernel<true, true>), grid, dim3(KID_LOWC_BLOCK), 0, stream, d_text, d_recs, (const uint64_t *)nullptr,
                           n, (uint32_t)parts, (uint32_t)t, base_bits, plane->as<uint8_t>(), d_n_masked);
    else
        hipLaunchKernelGGL((kid_lowc_mark_kernel<false, true>), grid, dim3(KID_LOWC_BLOCK), 0, stream, d_text, (const KidFastqRec *)nullptr,
                           d_offsets, n, (uint32_t)parts, (uint32_t)t, base_bits, plane->as<uint8_t>(), d_n_masked);
    KID_HIP(hipGetLastError());
    hipLaunchKernelGGL(kid_lowc_apply_kernel, dim3(kid_grid_for(plane_bytes / 16, KID_LOWC_BLOCK, db->num_cu * 16)), dim3(KID_LOWC_BLOCK), 0,
                       stream, d_text, (const uint8_t *)plane->p, text_nbytes);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// In place on text resident in HBM.  The host does not see the lengths here, so no line is split: one lane per read,
// whatever its length (long records: kid_lowc_batch, or the FASTQ forms).
extern "C" int kid_lowc_batch_device(kid_db *db, void *d_bases, const void *d_offsets, uint64_t n_reads, int low_complexity,
                                     void *d_n_masked, void *stream)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    int rc = kid_lowc_check_t(low_complexity);
    if (rc != KID_OK) return rc;
    if (n_reads == 0 || low_complexity == 0) return KID_OK;
    if (!d_bases || !d_offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    return kid_lowc_launch(db, (uint8_t *)d_bases, 0, nullptr, (const uint64_t *)d_offsets, n_reads, 0, low_complexity, nullptr,
                           (unsigned long long *)d_n_masked, (hipStream_t)stream);
}

extern "C" int kid_lowc_batch(kid_db *db, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int low_complexity,
                              uint8_t *out_bases, uint64_t *n_masked)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    int rc = kid_lowc_check_t(low_complexity);
    if (rc != KID_OK) return rc;
    if (n_masked) *n_masked = 0;
    if (n_reads == 0) return KID_OK;
    if (!bases || !offsets || !out_bases) return kid_fail(KID_ERR_ARG, "null argument");
    uint64_t longest = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return kid_fail(KID_ERR_ARG, "offsets not monotone at read %llu", (unsigned long long)r);
        if (offsets[r + 1] - offsets[r] > longest) longest = offsets[r + 1] - offsets[r];
    }
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    if (low_complexity == 0 || nbytes == 0) { // off: the text as it is
        if (out_bases != bases && nbytes) memmove(out_bases + base0, bases + base0, nbytes);
        return KID_OK;
    }
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    std::vector<uint64_t> rel;
    const uint64_t *off = kid_rebased_offsets(offsets, n_reads, rel);
    KidDevBuf dseq, doff, dcnt, plane;
    KID_HIP(dseq.alloc(kid_text_bytes(nbytes)));
    KID_HIP(doff.alloc((n_reads + 1) * 8));
    KID_HIP(dcnt.alloc(8));
    rc = kid_upload_text(dseq, bases + base0, nbytes, 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpy(doff.p, off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    KID_HIP(hipMemset(dcnt.p, 0, 8));
    rc = kid_lowc_launch(db, dseq.as<uint8_t>(), nbytes, nullptr, doff.as<uint64_t>(), n_reads, longest, low_complexity, &plane,
                         dcnt.as<unsigned long long>(), 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out_bases + base0, dseq.p, nbytes, hipMemcpyDeviceToHost));
    if (n_masked) KID_HIP(hipMemcpy(n_masked, dcnt.p, 8, hipMemcpyDeviceToHost));
    return KID_OK;
}
