// kid_api_support.h -- call reads by k-mer support: kid_db_read_support* over the hit pass (kid_api_hits.h) and
// kid_support_kernel (kid_support.hip.h).  Included behind the sample handle: a tally counts into one.
#pragma once
#include "kid_api_hits.h"
#include "kid_support.hip.h"

static_assert(sizeof(kid_support) == sizeof(KidSupport), "kid_support is the device record");

// the elapsed time of the support kernel of the call before
static int kid_support_settle(KidHitsState *h)
{
    if (!h->sup_pending) return KID_OK;
    KID_HIP(hipEventSynchronize(h->sup_ev1.e));
    float ms = 0;
    KID_HIP(hipEventElapsedTime(&ms, h->sup_ev0.e, h->sup_ev1.e));
    h->sup_ms += ms;
    h->sup_pending = false;
    return KID_OK;
}

// the hits scratch, free: the kernels of the call before, hit pass and support kernel, are through
static int kid_support_state(kid_db *db, KidHitsState **out)
{
    int rc = kid_hits_state(db, out);
    if (rc != KID_OK) return rc;
    KidHitsState *h = *out;
    if (!h->sup_ev0.e) KID_HIP(h->sup_ev0.create());
    if (!h->sup_ev1.e) KID_HIP(h->sup_ev1.create());
    return kid_support_settle(h);
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
    const KidSupportTally none{nullptr, nullptr, nullptr};
    KID_HIP(hipEventRecord(h->sup_ev0.e, stream));
    kid_lift(db->d.rows != nullptr, [&](auto rows) {
        kid_lift(t != nullptr, [&](auto tally) {
            hipLaunchKernelGGL((kid_support_kernel<decltype(rows)::value, decltype(tally)::value>), grid, block, 0, stream, db->d, d_hit_offsets,
                               d_hits, d_n_kmers, n, rule, d_out, t ? *t : none);
        });
    });
    KID_HIP(hipGetLastError());
    KID_HIP(hipEventRecord(h->sup_ev1.e, stream));
    h->sup_pending = true;
    h->sup_calls++;
    h->sup_reads += n;
    return KID_OK;
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch (count, the number of hits read
// back, fill), the support kernel, 24 bytes per read back.  A tally's kernel goes into the sample's stream behind
// whatever the sample has queued (classify kernels, a hit-log pass: both write the counters it adds to).
static int kid_support_host_run(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles,
                                KidSupportRule rule, kid_support *out, kid_sample *tally)
{
    const uint64_t n = b.n;
    int rc;
    KID_HIP(kid_hits_ensure(h->out_offsets, (n + 1) * 8));
    KID_HIP(kid_hits_ensure(h->out_nk, n * 4));
    if (out) KID_HIP(kid_hits_ensure(h->out_support, n * sizeof(KidSupport)));
    uint64_t *d_total = reinterpret_cast<uint64_t *>(h->ctl() + 33);
    rc = kid_hits_launch(db, h, b, recs, max_tiles, h->out_offsets.as<uint64_t>(), h->out_nk.as<uint32_t>(), nullptr, 0, nullptr, 0, false);
    if (rc != KID_OK) return rc;
    uint64_t total = 0;
    KID_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, 0));
    KID_HIP(hipStreamSynchronize(0));
    if (total > 0) {
        KID_HIP(kid_hits_ensure(h->out_hits, total * sizeof(KidHit)));
        if ((rc = kid_hits_launch_fill(db, h, b, recs, max_tiles, h->out_hits.as<KidHit>(), total, 0)) != KID_OK) return rc;
    }
    if ((rc = kid_hits_close(h, n, 0)) != KID_OK) return rc;
    // what the prepare kernels refuse (a range outside its read, a short quality line) is refused before anything is counted
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    hipStream_t st = 0;
    KidSupportTally t{nullptr, nullptr, nullptr};
    if (tally) {
        st = tally->stream.s;
        if (tally->has_last_stream && tally->last_stream != st) {
            if (!tally->order_ev.e) KID_HIP(tally->order_ev.create(hipEventDisableTiming));
            KID_HIP(hipEventRecord(tally->order_ev.e, tally->last_stream));
            KID_HIP(hipStreamWaitEvent(st, tally->order_ev.e, 0));
        }
        tally->last_stream = st;
        tally->has_last_stream = true;
        t.gcount = tally->gcount.as<unsigned long long>();
        t.seen = tally->seen.as<uint32_t>();
        t.fastq_desc = recs ? h->desc.as<KidReadDesc>() : nullptr;
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
    if (!bases || !offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((start == nullptr) != (stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    int64_t max_kmers = 0;
    uint64_t max_tiles = 0;
    rc = kid_check_offsets_batch(offsets, start, stop, n_reads, db->info.k, &max_kmers, KID_HITS_TILE, &max_tiles);
    if (rc != KID_OK) return rc;
    rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_support_state(db, &h)) != KID_OK) return rc;
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    if ((rc = kid_hits_upload_text(h, bases + base0, nbytes)) != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->in_offsets, (n_reads + 1) * 8));
    std::vector<uint64_t> rel; // (a synchronous copy reads it)
    const uint64_t *off_src = kid_rebased_offsets(offsets, n_reads, rel);
    KID_HIP(hipMemcpy(h->in_offsets.p, off_src, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    if (start) {
        KID_HIP(kid_hits_ensure(h->in_start, n_reads * 4));
        KID_HIP(kid_hits_ensure(h->in_stop, n_reads * 4));
        KID_HIP(hipMemcpy(h->in_start.p, start, n_reads * 4, hipMemcpyHostToDevice));
        KID_HIP(hipMemcpy(h->in_stop.p, stop, n_reads * 4, hipMemcpyHostToDevice));
    }
    KidBatch b{};
    b.bases = h->in_bases.as<uint8_t>();
    b.offsets = h->in_offsets.as<uint64_t>();
    b.start = start ? h->in_start.as<int32_t>() : nullptr;
    b.stop = start ? h->in_stop.as<int32_t>() : nullptr;
    b.n = n_reads;
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
    if (!text || !recs) return kid_fail(KID_ERR_ARG, "null argument");
    uint64_t max_tiles = 0;
    rc = kid_check_fastq_block(recs, n_reads, text_nbytes, KID_HITS_TILE, &max_tiles);
    if (rc != KID_OK) return rc;
    rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_support_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_upload_text(h, text, text_nbytes)) != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->in_recs, n_reads * sizeof(KidFastqRec)));
    KID_HIP(kid_hits_ensure(h->trim_start, n_reads * 4));
    KID_HIP(kid_hits_ensure(h->trim_stop, n_reads * 4));
    KID_HIP(hipMemcpy(h->in_recs.p, recs, n_reads * sizeof(KidFastqRec), hipMemcpyHostToDevice));
    KidBatch b{};
    b.bases = h->in_bases.as<uint8_t>();
    b.start = h->trim_start.as<int32_t>(); // (outputs of the prepare kernel here)
    b.stop = h->trim_stop.as<int32_t>();
    b.n = n_reads;
    return kid_support_host_run(db, h, b, h->in_recs.as<KidFastqRec>(), max_tiles, KidSupportRule{min_hits, min_permille}, out, tally);
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
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    if (device_ms) *device_ms = 0;
    if (calls) *calls = 0;
    if (reads) *reads = 0;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = db->hits.get();
    if (!h) return KID_OK;
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    if ((rc = kid_support_settle(h)) != KID_OK) return rc;
    if (device_ms) *device_ms = h->sup_ms;
    if (calls) *calls = h->sup_calls;
    if (reads) *reads = h->sup_reads;
    h->sup_ms = 0; h->sup_calls = 0; h->sup_reads = 0;
    return KID_OK;
}
