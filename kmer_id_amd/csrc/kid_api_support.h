// kid_api_support.h -- call reads by k-mer support: kid_db_read_support* over the hit pass and kid_support_kernel
// (kid_support.hip.h).  The host-buffer forms check and stage their batch and run the hit pass with the functions of
// kid_api_hits.h (kid_hits_check_*, kid_hits_stage_*, kid_hits_host_pass); the support kernel has the second
// KidSpanTimer of the database's KidHitsState.  Included behind the sample handle: a tally counts into one.
#pragma once
#include "kid_api_hits.h"
#include "kid_support.hip.h"

static_assert(sizeof(kid_support) == sizeof(KidSupport), "kid_support is the device record");

// the hits scratch, free: the kernels of the call before, hit pass and support kernel, are through
static int kid_support_state(kid_db *db, KidHitsState **out)
{
    int rc = kid_hits_state(db, out);
    if (rc != KID_OK) return rc;
    return (*out)->support.settle();
}

static int kid_support_check_rule(uint32_t min_permille)
{
    if (min_permille > 1000u) return kid_fail(KID_ERR_ARG, "min_permille = %u is more than 1000", min_permille);
    return KID_OK;
}

static int kid_support_check_tally(const kid_db *db, const kid_sample *tally)
{
    if (!tally) return KID_OK;
    if (tally->db != db) return kid_fail(KID_ERR_ARG, "the tally is a sample of another kid_db");
    if (tally->ended) return kid_fail(KID_ERR_STATE, "tally after kid_sample_end without kid_sample_reset");
    return KID_OK;
}

// the support kernel of one batch on `stream` between the two events; t: null, or what a tally needs
static int kid_support_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers,
                              uint64_t n, KidSupportRule rule, KidSupport *d_out, const KidSupportTally *t, hipStream_t stream)
{
    const dim3 grid(kid_grid_for(n, 256, db->num_cu * 8)), block(256);
    const KidSupportTally none{nullptr, nullptr, nullptr, nullptr};
    int rc = h->support.begin(stream);
    if (rc != KID_OK) return rc;
    kid_lift(db->d.rows != nullptr, [&](auto rows) {
        kid_lift(t != nullptr, [&](auto tally) {
            kid_lift(t != nullptr && t->depth != nullptr, [&](auto depth) { // the depth form exists for a tally alone
                if constexpr (decltype(tally)::value || !decltype(depth)::value)
                    hipLaunchKernelGGL((kid_support_kernel<decltype(rows)::value, decltype(tally)::value, decltype(depth)::value>), grid, block, 0,
                                       stream, db->d, d_hit_offsets, d_hits, d_n_kmers, n, rule, d_out, t ? *t : none);
            });
        });
    });
    KID_HIP(hipGetLastError());
    return h->support.end(stream, n);
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch (kid_hits_host_pass, every hit
// filled in), the support kernel, 24 bytes per read back.  A tally's kernel goes into the sample's stream behind
// whatever the sample has queued (classify kernels, a hit-log pass: both write the counters it adds to).
static int kid_support_host_run(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles,
                                KidSupportRule rule, kid_support *out, kid_sample *tally)
{
    const uint64_t n = b.n;
    uint64_t total = 0;
    int rc;
    if (out) KID_HIP(kid_hits_ensure(h->out_support, n * sizeof(KidSupport)));
    if ((rc = kid_hits_host_pass(db, h, b, recs, max_tiles, KID_HITS_NO_LIMIT, &total)) != KID_OK) return rc;
    // what the prepare kernels refuse (a range outside its read, a short quality line) is refused before anything is counted
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    hipStream_t st = 0;
    KidSupportTally t{nullptr, nullptr, nullptr, nullptr};
    if (tally) {
        st = tally->stream.s;
        if ((rc = kid_sample_order_behind(tally, st)) != KID_OK) return rc;
        t.gcount = tally->gcount.as<unsigned long long>();
        t.seen = tally->seen.as<uint32_t>();
        t.fastq_desc = recs ? h->desc.as<KidReadDesc>() : nullptr;
        t.depth = tally->depth.as<uint32_t>(); // null unless KID_OPT_ENTRY_DEPTH is on
    }
    rc = kid_support_launch(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), n, rule,
                            out ? h->out_support.as<KidSupport>() : nullptr, tally ? &t : nullptr, st);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(st));
    if (out) KID_HIP(hipMemcpy(out, h->out_support.p, n * sizeof(KidSupport), hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_db_read_support(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                   uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc != KID_OK) return rc;
    if ((rc = kid_support_check_tally(db, tally)) != KID_OK) return rc;
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (n_reads == 0) return KID_OK;
    uint64_t max_tiles = 0;
    if ((rc = kid_hits_check_offsets(db, bases, offsets, start, stop, n_reads, &max_tiles)) != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    KidBatch b{};
    if ((rc = kid_support_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_stage_offsets(h, bases, offsets, start, stop, n_reads, &b)) != KID_OK) return rc;
    return kid_support_host_run(db, h, b, nullptr, max_tiles, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_read_support_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                         uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc != KID_OK) return rc;
    if ((rc = kid_support_check_tally(db, tally)) != KID_OK) return rc;
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (n_reads == 0) return KID_OK;
    uint64_t max_tiles = 0;
    uint32_t longest = 0;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    if ((rc = kid_hits_check_fastq(db, text, text_nbytes, recs, n_reads, &max_tiles, &longest)) != KID_OK) return rc;
    KidHitsState *h = nullptr;
    KidBatch b{};
    const KidFastqRec *d_recs = nullptr;
    if ((rc = kid_support_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_stage_fastq(db, h, text, text_nbytes, recs, n_reads, longest, &b, &d_recs)) != KID_OK) return rc;
    return kid_support_host_run(db, h, b, d_recs, max_tiles, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_support_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                               uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc != KID_OK) return rc;
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (n_reads && (!d_hit_offsets || !d_n_kmers || !d_out)) return kid_fail(KID_ERR_ARG, "null argument");
    rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_support_state(db, &h)) != KID_OK) return rc;
    return kid_support_launch(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers, n_reads,
                              KidSupportRule{min_hits, min_permille}, (KidSupport *)d_out, nullptr, (hipStream_t)stream);
}

extern "C" int kid_db_read_support_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, &KidHitsState::support, false, device_ms, calls, reads);
}
