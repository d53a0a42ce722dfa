// kid_api_mask.h -- mask low-quality bases (kid_mask.hip.h): the range check of Q, the two launches of kid_mask_kernel
// (a FASTQ block with its line index: kid_classify_fastq_async and the FASTQ forms of kid_db_read_hits* /
// kid_db_read_support* run it on their device copy of the text; bases + quals + offsets: the unit entry points), the
// database's options (this one and KID_DB_OPT_LOW_COMPLEXITY, kid_api_lowc.h), and kid_mask_batch /
// kid_mask_batch_device.  The sample's option and counter are with the sample (kid_api.hip).
#pragma once
#include "kid_api_db.h"
#include "kid_api_lowc.h"
#include "kid_mask.hip.h"

#define KID_MAX_BASE_QUALITY 93 // '~' - 33: the highest quality a FASTQ line can spell

static int kid_mask_check_q(int q)
{
    if (q < 0 || q > KID_MAX_BASE_QUALITY) return kid_fail(KID_ERR_ARG, "min_base_quality = %d outside [0, %d]", q, KID_MAX_BASE_QUALITY);
    return KID_OK;
}

// A FASTQ block in HBM (text, its records), q > 0, on `stream`.  longest: the longest sequence line of the block, which
// decides into how many parts every record is split (kid_mask.hip.h): one per 2048 bases, at most 256.
static int kid_mask_launch_fastq(const kid_db *db, uint8_t *d_text, const KidFastqRec *d_recs, uint64_t n, uint32_t longest, int q,
                                 unsigned long long *d_n_masked, hipStream_t stream)
{
    uint32_t parts = longest / 2048u;
    parts = parts < 1u ? 1u : parts > 256u ? 256u : parts;
    const dim3 grid(kid_grid_for(n, KID_MASK_BLOCK / KID_MASK_TEAM, db->num_cu * 16), parts);
    hipLaunchKernelGGL(kid_mask_kernel<true>, grid, dim3(KID_MASK_BLOCK), 0, stream, d_text, (const uint8_t *)d_text, d_recs,
                       (const uint64_t *)nullptr, n, (uint32_t)q + 33u, d_n_masked);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// bases + quals + offsets in HBM, q > 0, n > 0, on `stream`.  nbytes: the size of the text when the host knows it
// (it sizes the grid), 0 when only the device does.
static int kid_mask_launch_offsets(const kid_db *db, uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n,
                                   uint64_t nbytes, int q, unsigned long long *d_n_masked, hipStream_t stream)
{
    const int grid = nbytes ? kid_grid_for(nbytes / 16 + 1, KID_MASK_BLOCK, db->num_cu * 16) : db->num_cu * 8;
    hipLaunchKernelGGL(kid_mask_kernel<false>, dim3(grid), dim3(KID_MASK_BLOCK), 0, stream, d_bases, d_quals, (const KidFastqRec *)nullptr,
                       d_offsets, n, (uint32_t)q + 33u, d_n_masked);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

extern "C" int kid_db_set_option(kid_db *db, int option, int value)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    switch (option) {
    case KID_DB_OPT_MIN_BASE_QUALITY: {
        int rc = kid_mask_check_q(value);
        if (rc != KID_OK) return rc;
        std::lock_guard<std::mutex> lock(db->hits_mu); // (the calls it applies to read it under the same lock)
        db->min_base_quality = value;
        return KID_OK;
    }
    case KID_DB_OPT_LOW_COMPLEXITY: {
        int rc = kid_lowc_check_t(value);
        if (rc != KID_OK) return rc;
        std::lock_guard<std::mutex> lock(db->hits_mu);
        db->low_complexity = value;
        return KID_OK;
    }
    default: return kid_fail(KID_ERR_ARG, "unknown option %d", option);
    }
}

extern "C" int kid_mask_batch_device(kid_db *db, void *d_bases, const void *d_quals, const void *d_offsets, uint64_t n_reads,
                                     int min_base_quality, void *d_n_masked, void *stream)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    int rc = kid_mask_check_q(min_base_quality);
    if (rc != KID_OK) return rc;
    if (n_reads == 0 || min_base_quality == 0) return KID_OK;
    if (!d_bases || !d_quals || !d_offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    return kid_mask_launch_offsets(db, (uint8_t *)d_bases, (const uint8_t *)d_quals, (const uint64_t *)d_offsets, n_reads, 0, min_base_quality,
                                   (unsigned long long *)d_n_masked, (hipStream_t)stream);
}

extern "C" int kid_mask_batch(kid_db *db, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads,
                              int min_base_quality, uint8_t *out_bases, uint64_t *n_masked)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    int rc = kid_mask_check_q(min_base_quality);
    if (rc != KID_OK) return rc;
    if (n_masked) *n_masked = 0;
    if (n_reads == 0) return KID_OK;
    if (!bases || !quals || !offsets || !out_bases) return kid_fail(KID_ERR_ARG, "null argument");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] < offsets[r]) return kid_fail(KID_ERR_ARG, "offsets not monotone at read %llu", (unsigned long long)r);
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    if (min_base_quality == 0 || nbytes == 0) { // off: the text as it is
        if (out_bases != bases && nbytes) memmove(out_bases + base0, bases + base0, nbytes);
        return KID_OK;
    }
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    // the reads lie back to back: to the kernel the batch is the one span [0, nbytes) of the uploaded text
    const uint64_t span[3] = {0, nbytes, 0}; // ([2]: the counter)
    KidDevBuf dseq, dq, dspan;
    KID_HIP(dseq.alloc(nbytes));
    KID_HIP(dq.alloc(nbytes));
    KID_HIP(dspan.alloc(sizeof(span)));
    KID_HIP(hipMemcpy(dseq.p, bases + base0, nbytes, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(dq.p, quals + base0, nbytes, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(dspan.p, span, sizeof(span), hipMemcpyHostToDevice));
    rc = kid_mask_launch_offsets(db, dseq.as<uint8_t>(), dq.as<uint8_t>(), dspan.as<uint64_t>(), 1, nbytes, min_base_quality,
                                 dspan.as<unsigned long long>() + 2, 0);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out_bases + base0, dseq.p, nbytes, hipMemcpyDeviceToHost));
    if (n_masked) KID_HIP(hipMemcpy(n_masked, dspan.as<uint64_t>() + 2, 8, hipMemcpyDeviceToHost));
    return KID_OK;
}
