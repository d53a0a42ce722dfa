// kid_api_segments.h -- call records in segments: kid_db_read_segments* over the hit pass and the kernels of
// kid_segments.hip.h -- and, once, the three forms of every family of segment calls (kid_segment_calls_*; the other
// family is kid_api_segment_votes.h's).  The host-buffer forms open their batch and run the hit pass with the functions of kid_api_hits.h
// (kid_hits_open_*, kid_hits_host_pass with every hit filled in); the device form runs kid_hits_launch into the caller's
// hit buffer.  While one of these calls runs, the hit pass also leaves the tiles' valid masks (KidHitsState::want_valid,
// sized by kid_segments_size).  The segment kernels -- segments per read and their scan, the scan of the valid masks
// (both kid_hits_scan), kid_segments_kernel -- follow the pass on its stream and have the KidSpanTimer of the family's
// KidFamilyState.  A call settles the pass, what every call waits for (KID_SETTLE_ALWAYS) and the support timer.
#pragma once
#include "kid_api_support.h"
#include "kid_segments.hip.h"

static_assert(sizeof(kid_segment) == sizeof(KidSegment) && sizeof(KidSegment) == 32, "kid_segment is the device record");

static int kid_segments_check_rule(uint32_t seg_len, uint32_t seg_step, uint32_t min_permille)
{
    if (seg_len == 0 || seg_step == 0) return kid_fail(KID_ERR_ARG, "seg_len and seg_step must be at least 1");
    if (seg_step > seg_len) return kid_fail(KID_ERR_ARG, "seg_step = %u is more than seg_len = %u (positions would be skipped)", seg_step, seg_len);
    if ((uint64_t)seg_len > (uint64_t)KID_SEGMENT_MAX_OVERLAP * seg_step)
        return kid_fail(KID_ERR_ARG, "seg_len = %u is more than %u * seg_step = %u", seg_len, KID_SEGMENT_MAX_OVERLAP, seg_step);
    return kid_support_check_rule(min_permille);
}

// What a segments call sizes between the state and the staging (KidHitsMoreScratch): room for the valid masks of a
// batch of up to max_tiles tiles and for their scan, the two totals.  The call then sets want_valid for its length.
static int kid_segments_size(KidHitsState *h, uint64_t max_tiles)
{
    if (!h->seg_ctl.p) {
        KID_HIP(h->seg_ctl.alloc(16));
        KID_HIP(hipMemset(h->seg_ctl.p, 0, 16));
    }
    KID_HIP(kid_hits_ensure(h->tile_valid, (max_tiles + 1) * 8));
    KID_HIP(kid_hits_ensure(h->tile_valid_off, (max_tiles + 1) * 8));
    return KID_OK;
}
struct KidWantValid { // (set for the length of a call, under the database's lock)
    KidHitsState *h;
    explicit KidWantValid(KidHitsState *s) : h(s) { h->want_valid = true; }
    ~KidWantValid() { h->want_valid = false; }
};

// behind the hit pass of batch b on `stream`: d_seg_offsets[n + 1] and the valid windows in front of every tile
static int kid_segments_launch_scans(kid_db *db, KidHitsState *h, uint64_t n, uint64_t max_tiles, KidSegGeom g, uint64_t *d_seg_offsets,
                                     hipStream_t stream)
{
    const int cu = db->num_cu;
    const uint64_t *n_tiles = reinterpret_cast<const uint64_t *>(h->ctl() + 32);
    uint64_t *totals = h->seg_ctl.as<uint64_t>();
    hipLaunchKernelGGL(kid_segments_count_kernel, dim3(kid_grid_for(n, 256, cu * 8)), dim3(256), 0, stream,
                       (const KidReadDesc *)h->desc.as<KidReadDesc>(), (const uint64_t *)h->tile_off.as<uint64_t>(), n, g, d_seg_offsets);
    kid_hits_scan<2>(cu, stream, d_seg_offsets, nullptr, n, d_seg_offsets, h->rsum.as<uint64_t>(), totals);
    kid_hits_scan<1>(cu, stream, h->tile_valid.p, n_tiles, max_tiles, h->tile_valid_off.as<uint64_t>(), h->tsum.as<uint64_t>(), totals + 1);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// A family of segment calls -- KidSegmentCalls here, KidSegmentVoteCalls in kid_api_segment_votes.h -- is a struct with
//   Rec      its device record (= the C ABI's)
//   id       its KidFamilyState in KidHitsState: the host forms' records, the timer of its kernels
//   settle   the timers it waits for before the scratch is its own (kid_hits_state)
//   launch   its kernels behind the scans over the batch `a` on `stream`, the grid sized for a.seg_cap segments
// and kid_segment_calls_* below are its three forms, once: the checks, the hit pass, the scans, the launch, the downloads.
struct KidSegmentCalls {
    typedef KidSegment Rec;
    static constexpr KidFamily id = KID_FAM_SEGMENTS;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT);
    static int launch(kid_db *db, KidHitsState *, const KidSegmentsIn &a, KidSegGeom g, KidSupportRule rule, KidSegment *d_segments,
                      hipStream_t stream)
    {
        const dim3 grid(kid_grid_for(a.seg_cap, 256, db->num_cu * 8)), block(256);
        kid_lift(db->d.rows != nullptr, [&](auto rows) {
            hipLaunchKernelGGL((kid_segments_kernel<decltype(rows)::value>), grid, block, 0, stream, db->d, a, g, rule, d_segments);
        });
        return KID_OK;
    }
};

// seg_cap: what the caller's buffer holds, and what the grid is sized for (the kernels stride over whatever the batch has)
template <class F>
static int kid_segment_calls_launch(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, KidSegGeom g, KidSupportRule rule,
                                    const uint64_t *d_seg_offsets, const KidHit *d_hits, uint64_t hits_cap, typename F::Rec *d_segments,
                                    uint64_t seg_cap, hipStream_t stream)
{
    KidSegmentsIn a{};
    a.desc = h->desc.as<KidReadDesc>();
    a.tile_off = h->tile_off.as<uint64_t>();
    a.seg_offsets = d_seg_offsets;
    a.n_reads = b.n;
    a.tile_mask = h->tile_mask.as<unsigned long long>();
    a.tile_valid = h->tile_valid.as<unsigned long long>();
    a.tile_hit_off = h->tile_hit_off.as<uint64_t>();
    a.tile_valid_off = h->tile_valid_off.as<uint64_t>();
    a.hits = d_hits;
    a.offsets = b.offsets;
    a.recs = recs;
    a.hits_cap = hits_cap;
    a.seg_cap = seg_cap;
    const int rc = F::launch(db, h, a, g, rule, d_segments, stream);
    if (rc != KID_OK) return rc;
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch, the scans, the number of
// segments read back, the kernels if the caller's buffer holds them, downloads.
template <class F>
static int kid_segment_calls_host_run(kid_db *db, const KidOpenBatch &ob, KidSegGeom g, KidSupportRule rule, uint64_t *seg_offsets, void *segments,
                                      uint64_t cap, uint64_t *n_segments)
{
    typedef typename F::Rec Rec;
    KidHitsState *h = ob.h;
    KidSpanTimer &timer = h->family[F::id].timer;
    KidDevBuf &d_out = h->family[F::id].out;
    const KidWantValid valid(h);
    const uint64_t n = ob.b.n, limit = segments ? cap : 0;
    uint64_t n_hits = 0, total = 0;
    int rc;
    KID_HIP(kid_hits_ensure(h->out_seg_offsets, (n + 1) * 8));
    if ((rc = kid_hits_host_pass(db, ob, KID_HITS_NO_LIMIT, &n_hits)) != KID_OK) return rc;
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    uint64_t *d_seg_offsets = h->out_seg_offsets.as<uint64_t>();
    if ((rc = timer.begin(0)) != KID_OK) return rc;
    if ((rc = kid_segments_launch_scans(db, h, n, ob.max_tiles, g, d_seg_offsets, 0)) != KID_OK) return rc;
    KID_HIP(hipMemcpyAsync(&total, h->seg_ctl.p, 8, hipMemcpyDeviceToHost, 0));
    KID_HIP(hipStreamSynchronize(0));
    const bool fill = total > 0 && total <= limit;
    if (fill) {
        KID_HIP(kid_hits_ensure(d_out, total * sizeof(Rec)));
        rc = kid_segment_calls_launch<F>(db, h, ob.b, ob.d_recs, g, rule, d_seg_offsets, n_hits ? h->out_hits.as<KidHit>() : nullptr,
                                         KID_HITS_NO_LIMIT, d_out.as<Rec>(), total, 0);
        if (rc != KID_OK) return rc;
    }
    if ((rc = timer.end(0, n)) != KID_OK) return rc;
    KID_HIP(hipMemcpy(seg_offsets, d_seg_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (fill) KID_HIP(hipMemcpy(segments, d_out.p, total * sizeof(Rec), hipMemcpyDeviceToHost));
    *n_segments = total;
    return KID_OK;
}

template <class F>
static int kid_segment_calls_offsets(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                     uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                                     uint64_t *seg_offsets, void *segments, uint64_t cap, uint64_t *n_segments)
{
    int rc = kid_check_csr_out(db, seg_offsets, segments, cap, n_segments, n_reads, "segments");
    if (rc == KID_OK) rc = kid_segments_check_rule(seg_len, seg_step, min_permille);
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return kid_csr_out_empty(seg_offsets, n_segments);
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, F::settle, kid_segments_size)) != KID_OK) return rc;
    return kid_segment_calls_host_run<F>(db, ob, KidSegGeom{seg_len, seg_step}, KidSupportRule{min_hits, min_permille}, seg_offsets, segments, cap,
                                         n_segments);
}

template <class F>
static int kid_segment_calls_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                   uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille, uint64_t *seg_offsets,
                                   void *segments, uint64_t cap, uint64_t *n_segments)
{
    int rc = kid_check_csr_out(db, seg_offsets, segments, cap, n_segments, n_reads, "segments");
    if (rc == KID_OK) rc = kid_segments_check_rule(seg_len, seg_step, min_permille);
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return kid_csr_out_empty(seg_offsets, n_segments);
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, F::settle, kid_segments_size)) != KID_OK) return rc;
    return kid_segment_calls_host_run<F>(db, ob, KidSegGeom{seg_len, seg_step}, KidSupportRule{min_hits, min_permille}, seg_offsets, segments, cap,
                                         n_segments);
}

template <class F>
static int kid_segment_calls_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                    const void *d_stop, uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits,
                                    uint32_t min_permille, void *d_hits, uint64_t hits_cap, void *d_seg_offsets, void *d_segments,
                                    uint64_t seg_cap, void *d_n_hits, void *d_n_segments, void *stream)
{
    if (!db || !d_seg_offsets || !d_n_hits || !d_n_segments) return kid_fail(KID_ERR_ARG, "null argument");
    KidBatch b{};
    int rc = kid_check_device_batch(d_bases, d_offsets, d_start, d_stop, n_reads, &b);
    if (rc == KID_OK) rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (hits_cap && !d_hits) return kid_fail(KID_ERR_ARG, "hits_cap without a hits buffer");
    if (seg_cap && !d_segments) return kid_fail(KID_ERR_ARG, "seg_cap without a segments buffer");
    if ((rc = kid_segments_check_rule(seg_len, seg_step, min_permille)) != KID_OK) return rc;
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_reads == 0) return kid_csr_out_empty_device(st, d_seg_offsets, d_n_hits, d_n_segments);
    const uint64_t max_tiles = bases_nbytes / KID_HITS_TILE + n_reads;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, F::settle, &h)) != KID_OK) return rc;
    if ((rc = kid_segments_size(h, max_tiles)) != KID_OK) return rc;
    KidWantValid valid(h);
    KidSpanTimer &timer = h->family[F::id].timer;
    KID_HIP(kid_hits_ensure(h->out_offsets, (n_reads + 1) * 8)); // (the hit pass wants a place for its CSR offsets)
    rc = kid_hits_launch(db, h, b, nullptr, max_tiles, h->out_offsets.as<uint64_t>(), nullptr, (KidHit *)d_hits, hits_cap, (uint64_t *)d_n_hits, st, true);
    if (rc != KID_OK) return rc;
    if ((rc = h->pass.end(st, n_reads)) != KID_OK) return rc;
    const KidSegGeom g{seg_len, seg_step};
    if ((rc = timer.begin(st)) != KID_OK) return rc;
    if ((rc = kid_segments_launch_scans(db, h, n_reads, max_tiles, g, (uint64_t *)d_seg_offsets, st)) != KID_OK) return rc;
    KID_HIP(hipMemcpyAsync(d_n_segments, h->seg_ctl.p, 8, hipMemcpyDeviceToDevice, st));
    if (seg_cap) {
        rc = kid_segment_calls_launch<F>(db, h, b, nullptr, g, KidSupportRule{min_hits, min_permille}, (const uint64_t *)d_seg_offsets,
                                         (const KidHit *)d_hits, hits_cap, (typename F::Rec *)d_segments, seg_cap, st);
        if (rc != KID_OK) return rc;
    }
    return timer.end(st, n_reads);
}

extern "C" int kid_db_read_segments(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                    uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                                    uint64_t *seg_offsets, kid_segment *segments, uint64_t cap, uint64_t *n_segments)
{
    return kid_segment_calls_offsets<KidSegmentCalls>(db, bases, offsets, start, stop, n_reads, seg_len, seg_step, min_hits, min_permille,
                                                      seg_offsets, segments, cap, n_segments);
}

extern "C" int kid_db_read_segments_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                          uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille, uint64_t *seg_offsets,
                                          kid_segment *segments, uint64_t cap, uint64_t *n_segments)
{
    return kid_segment_calls_fastq<KidSegmentCalls>(db, text, text_nbytes, recs, n_reads, seg_len, seg_step, min_hits, min_permille, seg_offsets,
                                                    segments, cap, n_segments);
}

extern "C" int kid_db_read_segments_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                           const void *d_stop, uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits,
                                           uint32_t min_permille, void *d_hits, uint64_t hits_cap, void *d_seg_offsets, void *d_segments,
                                           uint64_t seg_cap, void *d_n_hits, void *d_n_segments, void *stream)
{
    return kid_segment_calls_device<KidSegmentCalls>(db, d_bases, bases_nbytes, d_offsets, d_start, d_stop, n_reads, seg_len, seg_step, min_hits,
                                                     min_permille, d_hits, hits_cap, d_seg_offsets, d_segments, seg_cap, d_n_hits, d_n_segments,
                                                     stream);
}

extern "C" int kid_db_read_segments_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KidSegmentCalls::id, device_ms, calls, reads);
}
