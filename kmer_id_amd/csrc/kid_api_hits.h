// kid_api_hits.h -- every read's k-mer hits: the scratch of a database's hit passes and kid_db_read_hits*.
// What the host-buffer forms of kid_db_read_support* (kid_api_support.h) share with those of kid_db_read_hits* is here
// once: KidSpanTimer, the argument checks and the staging of a batch (kid_hits_check_* / kid_hits_stage_*, one pair per
// input form) and the hit pass into the library's own buffers (kid_hits_host_pass).
#pragma once
#include "kid_api_db.h"
#include "kid_api_mask.h"
#include "kid_hits.hip.h"

// ---------------------------------------------------------------- every read's k-mer hits (kid_hits.hip.h)
// Scratch of the hit pass: grow-only device buffers sized by the largest batch seen, one set per database (calls on
// one kid_db run one after the other: a call first waits for the kernels of the call before).  Per batch: 16 B per
// read (descriptors) + 8 B per read (first tile) + 16 B per tile of 64 windows (mask, first hit) + 8 B per 1024 of
// either (scan totals); the host-buffer forms add a device copy of their inputs and outputs.  kid_db_read_segments* add
// 16 B per tile (valid mask, its scan), 8 B per read (first segment) and 32 B per segment (host forms).
// The device time between two events on a stream, added up over the calls since somebody took it
struct __attribute__((visibility("hidden"))) KidSpanTimer {
    KidEvent ev0, ev1;
    bool pending = false;
    double ms = 0;
    uint64_t calls = 0, reads = 0;
    hipError_t create()
    {
        const hipError_t e = ev0.create();
        return e != hipSuccess ? e : ev1.create();
    }
    int begin(hipStream_t stream)
    {
        KID_HIP(hipEventRecord(ev0.e, stream));
        return KID_OK;
    }
    int end(hipStream_t stream, uint64_t n_reads)
    {
        KID_HIP(hipEventRecord(ev1.e, stream));
        pending = true;
        calls++;
        reads += n_reads;
        return KID_OK;
    }
    // the elapsed time of the span before (and with it: what ran inside it is through)
    int settle()
    {
        if (!pending) return KID_OK;
        KID_HIP(hipEventSynchronize(ev1.e));
        float span = 0;
        KID_HIP(hipEventElapsedTime(&span, ev0.e, ev1.e));
        ms += span;
        pending = false;
        return KID_OK;
    }
    void take(double *device_ms, uint64_t *n_calls, uint64_t *n_reads)
    {
        if (device_ms) *device_ms = ms;
        if (n_calls) *n_calls = calls;
        if (n_reads) *n_reads = reads;
        ms = 0; calls = 0; reads = 0;
    }
};

struct KidHitsState {
    KidDevBuf desc, tile_off, rsum, tile_mask, tile_hit_off, tsum, trim_start, trim_stop;          // every form
    KidDevBuf in_bases, in_offsets, in_start, in_stop, in_recs, out_offsets, out_nk, out_hits;      // host-buffer forms
    // unsigned long long [0..31] the `stats` block the prepare kernels write ([4] ranges outside the read, [8] short
    // quality lines), [32] tiles of the batch, [33] hits of the batch, [34] sink for the prepare kernel's gcount
    // correction, [35] batches with more tiles than the scratch was sized for,
    // then a KidRareArgs (the prepare kernels announce the batch's longest read there; nobody reads it)
    KidDevBuf ctl_buf;
    uint32_t seq = 0;
    KidDevBuf out_support; // kid_db_read_support* (kid_api_support.h): the host forms' records
    KidSpanTimer pass;     // the hit pass of every call, a kid_db_read_support* host call's included
    KidSpanTimer support;  // the support kernel alone
    KidDevBuf out_fragments; // kid_db_read_fragments* (kid_api_fragments.h): the host forms' records
    KidSpanTimer fragments;  // the fragment kernel alone
    // kid_db_read_segments* (kid_api_segments.h): per tile the mask of its lanes that hold a k-mer and their scan (the hit
    // pass stores the mask while want_valid is set: the buffer is sized for the batch then), [0] the batch's segments and
    // [1] its valid windows, the host forms' offsets and records
    KidDevBuf tile_valid, tile_valid_off, seg_ctl, out_seg_offsets, out_segments;
    bool want_valid = false;
    KidSpanTimer segments; // the segment kernels alone
    unsigned long long *ctl() const { return ctl_buf.as<unsigned long long>(); }
};
#define KID_HITS_CTL_WORDS 36u

kid_db::~kid_db() {}

// a little slack: batches of a file differ slightly in size
static hipError_t kid_hits_ensure(KidDevBuf &b, uint64_t nbytes) { return b.ensure(nbytes, ((nbytes + nbytes / 8) + 255u) & ~255ull); }

// the scratch, free: the hit pass of the call before, and the segment kernels behind it, are through
static int kid_hits_state(kid_db *db, KidHitsState **out)
{
    if (!db->hits) {
        std::unique_ptr<KidHitsState> h(new KidHitsState());
        const size_t nb = KID_HITS_CTL_WORDS * 8 + sizeof(KidRareArgs);
        KID_HIP(h->ctl_buf.alloc(nb));
        KID_HIP(hipMemset(h->ctl(), 0, nb));
        KID_HIP(h->pass.create());
        KID_HIP(h->support.create());
        KID_HIP(h->fragments.create());
        KID_HIP(h->segments.create());
        db->hits = std::move(h);
    }
    *out = db->hits.get();
    const int rc = (*out)->pass.settle();
    return rc != KID_OK ? rc : (*out)->segments.settle(); // (the segment kernels read the tiles' scratch behind the pass)
}

static KidHitsTiles kid_hits_tiles(const KidHitsState *h, const KidBatch &b)
{
    KidHitsTiles a{};
    a.bases = b.bases;
    a.desc = h->desc.as<KidReadDesc>();
    a.tile_off = h->tile_off.as<uint64_t>();
    a.n_reads = b.n;
    a.tile_mask = h->tile_mask.as<unsigned long long>();
    a.tile_valid = h->want_valid ? h->tile_valid.as<unsigned long long>() : nullptr;
    return a;
}

// the fill pass on its own: the host-buffer forms learn the number of hits first and then size their device buffer
static int kid_hits_launch_fill(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles, KidHit *d_hits,
                                uint64_t cap, hipStream_t stream)
{
    hipLaunchKernelGGL(kid_hits_fill_kernel, dim3(kid_grid_for(max_tiles, KID_HITS_WG_TILES, db->num_cu * 32)), dim3(256), 0, stream, db->d,
                       kid_hits_tiles(h, b), (const uint64_t *)h->tile_hit_off.as<uint64_t>(), b.offsets, recs, d_hits, cap);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// The kernels of one batch on `stream`, everything on the device.  b: bases / offsets / start / stop (recs: a FASTQ
// block instead, start and stop are then outputs of the prepare kernel).  max_tiles: see below.
static int kid_hits_launch(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles,
                           uint64_t *d_hit_offsets, uint32_t *d_n_kmers, KidHit *d_hits, uint64_t cap, uint64_t *d_n_hits,
                           hipStream_t stream, bool fill)
{
    const uint64_t n = b.n;
    // max_tiles: what the tile arrays are sized for.  A read of L bytes has at most L / 64 + 1 tiles: the host-buffer
    // forms add that up over their reads; the device form knows the text's size alone and takes bytes / 64 + reads, which
    // holds unless reads overlap.  A batch with more tiles is refused on the device (kid_hits_scan_top_kernel).
    KID_HIP(kid_hits_ensure(h->desc, n * sizeof(KidReadDesc)));
    KID_HIP(kid_hits_ensure(h->tile_off, (n + 1) * 8));
    KID_HIP(kid_hits_ensure(h->rsum, (n / KID_HITS_SCAN_BLOCK + 2) * 8));
    KID_HIP(kid_hits_ensure(h->tile_mask, (max_tiles + 1) * 8));
    KID_HIP(kid_hits_ensure(h->tile_hit_off, (max_tiles + 1) * 8));
    KID_HIP(kid_hits_ensure(h->tsum, (max_tiles / KID_HITS_SCAN_BLOCK + 2) * 8));
    unsigned long long *stats = h->ctl();
    uint64_t *n_tiles = reinterpret_cast<uint64_t *>(h->ctl() + 32), *n_hits = reinterpret_cast<uint64_t *>(h->ctl() + 33);
    KidRareArgs *rare = reinterpret_cast<KidRareArgs *>(h->ctl() + KID_HITS_CTL_WORDS);
    KidReadDesc *desc = h->desc.as<KidReadDesc>();
    uint64_t *tile_off = h->tile_off.as<uint64_t>(), *tile_hit_off = h->tile_hit_off.as<uint64_t>();
    const int cu = db->num_cu;
    int rc = h->pass.begin(stream);
    if (rc != KID_OK) return rc;
    if (recs)
        hipLaunchKernelGGL(kid_prepare_fastq_kernel, dim3(kid_grid_for(n, 256, cu * 8)), dim3(256), 0, stream, b.bases, recs, n, db->info.k,
                           desc, const_cast<int32_t *>(b.start), const_cast<int32_t *>(b.stop), (uint32_t *)nullptr, stats, h->ctl() + 34, rare,
                           ++h->seq, 0);
    else
        hipLaunchKernelGGL(kid_prepare_kernel, dim3(kid_grid_for(n, 256, cu * 8)), dim3(256), 0, stream, b, db->info.k, desc, stats, rare,
                           ++h->seq, 0u, (KidLongList *)nullptr, 0);
    // tiles per read -> first tile of every read (n_kmers is cleared on the way)
    hipLaunchKernelGGL(kid_hits_scan_local_kernel<0>, dim3(kid_grid_for(n, KID_HITS_SCAN_BLOCK, cu * 8)), dim3(256), 0, stream,
                       (const void *)desc, (const uint64_t *)nullptr, n, tile_off, h->rsum.as<uint64_t>(), d_n_kmers);
    hipLaunchKernelGGL(kid_hits_scan_top_kernel, dim3(1), dim3(1024), 0, stream, h->rsum.as<uint64_t>(), (const uint64_t *)nullptr, n, n_tiles,
                       max_tiles, h->ctl() + 35);
    hipLaunchKernelGGL(kid_hits_scan_add_kernel, dim3(kid_grid_for(n, 256, cu * 8)), dim3(256), 0, stream, tile_off,
                       (const uint64_t *)h->rsum.as<uint64_t>(), (const uint64_t *)nullptr, n, (const uint64_t *)n_tiles);
    const KidHitsTiles a = kid_hits_tiles(h, b);
    const int tile_grid = kid_grid_for(max_tiles, KID_HITS_WG_TILES, cu * 32);
    hipLaunchKernelGGL(kid_hits_count_kernel, dim3(tile_grid), dim3(256), 0, stream, db->d, a, d_n_kmers);
    // hits per tile -> first hit of every tile
    hipLaunchKernelGGL(kid_hits_scan_local_kernel<1>, dim3(kid_grid_for(max_tiles, KID_HITS_SCAN_BLOCK, cu * 8)), dim3(256), 0, stream,
                       (const void *)a.tile_mask, (const uint64_t *)n_tiles, 0ull, tile_hit_off, h->tsum.as<uint64_t>(), (uint32_t *)nullptr);
    hipLaunchKernelGGL(kid_hits_scan_top_kernel, dim3(1), dim3(1024), 0, stream, h->tsum.as<uint64_t>(), (const uint64_t *)n_tiles, 0ull, n_hits,
                       ~0ull, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(kid_hits_scan_add_kernel, dim3(kid_grid_for(max_tiles, 256, cu * 8)), dim3(256), 0, stream, tile_hit_off,
                       (const uint64_t *)h->tsum.as<uint64_t>(), (const uint64_t *)n_tiles, 0ull, (const uint64_t *)n_hits);
    hipLaunchKernelGGL(kid_hits_offsets_kernel, dim3(kid_grid_for(n + 1, 256, cu * 8)), dim3(256), 0, stream, (const uint64_t *)tile_off,
                       (const uint64_t *)tile_hit_off, n, d_hit_offsets, d_n_hits);
    if (fill && d_hits && cap) return kid_hits_launch_fill(db, h, b, recs, max_tiles, d_hits, cap, stream);
    KID_HIP(hipGetLastError());
    return KID_OK;
}

// what the prepare kernels found wrong with the batch just run (host-buffer forms: after the kernels)
static int kid_hits_check(KidHitsState *h)
{
    unsigned long long st[KID_HITS_CTL_WORDS];
    KID_HIP(hipMemcpy(st, h->ctl(), sizeof(st), hipMemcpyDeviceToHost));
    if (st[4] == 0 && st[8] == 0 && st[35] == 0) return KID_OK;
    KID_HIP(hipMemset(h->ctl(), 0, KID_HITS_CTL_WORDS * 8));
    if (st[35] != 0)
        return kid_fail(KID_ERR_ARG, "%llu batches held more windows than their text has bytes (reads that overlap, or a text longer than "
                                     "bases_nbytes): they were given no hits", st[35]);
    if (st[4] != 0)
        return kid_fail(KID_ERR_ARG, "%llu reads had [start,stop] outside the read (string::at would throw)", st[4]);
    return kid_fail(KID_ERR_FORMAT, "%llu FASTQ records have a quality line shorter than the sequence (qual.at() throws in the reference)", st[8]);
}

// The hit pass of a host-buffer form into the library's own buffers (out_offsets, out_nk, out_hits) on stream 0: the
// count pass, the number of hits read back, the fill pass if that number is neither 0 nor more than `limit`.
#define KID_HITS_NO_LIMIT (~0ull)
static int kid_hits_host_pass(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles, uint64_t limit,
                              uint64_t *n_hits)
{
    const uint64_t n = b.n;
    int rc;
    KID_HIP(kid_hits_ensure(h->out_offsets, (n + 1) * 8));
    KID_HIP(kid_hits_ensure(h->out_nk, n * 4));
    uint64_t *d_total = reinterpret_cast<uint64_t *>(h->ctl() + 33);
    rc = kid_hits_launch(db, h, b, recs, max_tiles, h->out_offsets.as<uint64_t>(), h->out_nk.as<uint32_t>(), nullptr, 0, nullptr, 0, false);
    if (rc != KID_OK) return rc;
    uint64_t total = 0;
    KID_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, 0));
    KID_HIP(hipStreamSynchronize(0));
    if (total > 0 && total <= limit) {
        KID_HIP(kid_hits_ensure(h->out_hits, total * sizeof(KidHit)));
        if ((rc = kid_hits_launch_fill(db, h, b, recs, max_tiles, h->out_hits.as<KidHit>(), total, 0)) != KID_OK) return rc;
    }
    *n_hits = total;
    return h->pass.end(0, n);
}

// the host-buffer forms behind their uploads: the hit pass, the fill if the caller's buffer holds it, downloads
static int kid_hits_host_run(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles, uint64_t *hit_offsets,
                             uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits)
{
    static_assert(sizeof(kid_hit) == sizeof(KidHit), "kid_hit is the device record");
    const uint64_t n = b.n, limit = hits ? cap : 0;
    uint64_t total = 0;
    int rc = kid_hits_host_pass(db, h, b, recs, max_tiles, limit, &total);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpy(hit_offsets, h->out_offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (n_kmers) KID_HIP(hipMemcpy(n_kmers, h->out_nk.p, n * 4, hipMemcpyDeviceToHost));
    if (total > 0 && total <= limit) KID_HIP(hipMemcpy(hits, h->out_hits.p, total * sizeof(KidHit), hipMemcpyDeviceToHost));
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    *n_hits = total;
    return KID_OK;
}

// The host-buffer forms, one pair of functions per input form.  kid_hits_check_*: what the host can refuse about the
// arguments of a batch that has reads, then the database's device selected; *max_tiles: what the tile arrays are sized
// for.  kid_hits_stage_*: the batch copied into the scratch (synchronous copies on stream 0) -> the KidBatch of the copy.
static int kid_hits_check_offsets(const kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                  uint64_t n_reads, uint64_t *max_tiles)
{
    if (!bases || !offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((start == nullptr) != (stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    int64_t max_kmers = 0;
    int rc = kid_check_offsets_batch(offsets, start, stop, n_reads, db->info.k, &max_kmers, KID_HITS_TILE, max_tiles);
    if (rc != KID_OK) return rc;
    return kid_use_device(db->device);
}

// (called with the database's lock held: db->min_base_quality, under which the block's lines must be in order; *longest:
// the longest sequence line, for the mask kernel)
static int kid_hits_check_fastq(const kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                uint64_t *max_tiles, uint32_t *longest)
{
    if (!text || !recs) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_check_fastq_block(recs, n_reads, text_nbytes, KID_HITS_TILE, max_tiles, db->min_base_quality > 0, longest);
    if (rc != KID_OK) return rc;
    return kid_use_device(db->device);
}

static int kid_hits_stage_text(KidHitsState *h, const uint8_t *src, uint64_t nbytes, KidBatch *b)
{
    KID_HIP(kid_hits_ensure(h->in_bases, kid_text_bytes(nbytes)));
    b->bases = h->in_bases.as<uint8_t>();
    return kid_upload_text(h->in_bases, src, nbytes, 0);
}

static int kid_hits_stage_offsets(KidHitsState *h, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                  uint64_t n_reads, KidBatch *b)
{
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    int rc = kid_hits_stage_text(h, bases + base0, nbytes, b);
    if (rc != KID_OK) return rc;
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
    b->offsets = h->in_offsets.as<uint64_t>();
    b->start = start ? h->in_start.as<int32_t>() : nullptr;
    b->stop = start ? h->in_stop.as<int32_t>() : nullptr;
    b->n = n_reads;
    return KID_OK;
}

// (under KID_DB_OPT_MIN_BASE_QUALITY the staged text is masked here, in front of the hit pass: the caller's is not touched)
static int kid_hits_stage_fastq(const kid_db *db, KidHitsState *h, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs,
                                uint64_t n_reads, uint32_t longest, KidBatch *b, const KidFastqRec **d_recs)
{
    int rc = kid_hits_stage_text(h, text, text_nbytes, b);
    if (rc != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->in_recs, n_reads * sizeof(KidFastqRec)));
    KID_HIP(kid_hits_ensure(h->trim_start, n_reads * 4));
    KID_HIP(kid_hits_ensure(h->trim_stop, n_reads * 4));
    KID_HIP(hipMemcpy(h->in_recs.p, recs, n_reads * sizeof(KidFastqRec), hipMemcpyHostToDevice));
    b->start = h->trim_start.as<int32_t>(); // (outputs of the prepare kernel here)
    b->stop = h->trim_stop.as<int32_t>();
    b->n = n_reads;
    *d_recs = h->in_recs.as<KidFastqRec>();
    if (db->min_base_quality > 0)
        return kid_mask_launch_fastq(db, h->in_bases.as<uint8_t>(), *d_recs, n_reads, longest, db->min_base_quality, nullptr, 0);
    return KID_OK;
}

extern "C" int kid_db_read_hits(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                uint64_t n_reads, uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits)
{
    if (!db || !hit_offsets || !n_hits) return kid_fail(KID_ERR_ARG, "null argument");
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (cap && !hits) return kid_fail(KID_ERR_ARG, "cap without a hits buffer");
    if (n_reads == 0) { hit_offsets[0] = 0; *n_hits = 0; return KID_OK; }
    uint64_t max_tiles = 0;
    int rc = kid_hits_check_offsets(db, bases, offsets, start, stop, n_reads, &max_tiles);
    if (rc != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    KidBatch b{};
    if ((rc = kid_hits_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_stage_offsets(h, bases, offsets, start, stop, n_reads, &b)) != KID_OK) return rc;
    return kid_hits_host_run(db, h, b, nullptr, max_tiles, hit_offsets, n_kmers, hits, cap, n_hits);
}

extern "C" int kid_db_read_hits_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                      uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits)
{
    if (!db || !hit_offsets || !n_hits) return kid_fail(KID_ERR_ARG, "null argument");
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (cap && !hits) return kid_fail(KID_ERR_ARG, "cap without a hits buffer");
    if (n_reads == 0) { hit_offsets[0] = 0; *n_hits = 0; return KID_OK; }
    uint64_t max_tiles = 0;
    uint32_t longest = 0;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    int rc = kid_hits_check_fastq(db, text, text_nbytes, recs, n_reads, &max_tiles, &longest);
    if (rc != KID_OK) return rc;
    KidHitsState *h = nullptr;
    KidBatch b{};
    const KidFastqRec *d_recs = nullptr;
    if ((rc = kid_hits_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_stage_fastq(db, h, text, text_nbytes, recs, n_reads, longest, &b, &d_recs)) != KID_OK) return rc;
    return kid_hits_host_run(db, h, b, d_recs, max_tiles, hit_offsets, n_kmers, hits, cap, n_hits);
}

extern "C" int kid_db_read_hits_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                       const void *d_stop, uint64_t n_reads, void *d_hit_offsets, void *d_n_kmers, void *d_hits,
                                       uint64_t cap, void *d_n_hits, void *stream)
{
    if (!db || !d_hit_offsets || !d_n_hits || (n_reads && (!d_bases || !d_offsets))) return kid_fail(KID_ERR_ARG, "null argument");
    if (((uintptr_t)d_bases & 15u) != 0) return kid_fail(KID_ERR_ARG, "d_bases must be 16-byte aligned");
    if ((d_start == nullptr) != (d_stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (cap && !d_hits) return kid_fail(KID_ERR_ARG, "cap without a hits buffer");
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_reads == 0) {
        KID_HIP(hipMemsetAsync(d_hit_offsets, 0, 8, st));
        KID_HIP(hipMemsetAsync(d_n_hits, 0, 8, st));
        return KID_OK;
    }
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, &h)) != KID_OK) return rc;
    KidBatch b{};
    b.bases = (const uint8_t *)d_bases;
    b.offsets = (const uint64_t *)d_offsets;
    b.start = (const int32_t *)d_start;
    b.stop = (const int32_t *)d_stop;
    b.n = n_reads;
    rc = kid_hits_launch(db, h, b, nullptr, bases_nbytes / KID_HITS_TILE + n_reads, (uint64_t *)d_hit_offsets, (uint32_t *)d_n_kmers, (KidHit *)d_hits, cap,
                         (uint64_t *)d_n_hits, st, true);
    if (rc != KID_OK) return rc;
    return h->pass.end(st, n_reads);
}

// kid_db_read_hits_time / kid_db_read_support_time: one of the state's timers, settled and taken; check: report what
// the prepare kernels refused since the last query as well
static int kid_hits_take_time(kid_db *db, KidSpanTimer KidHitsState::*timer, bool check, double *device_ms, uint64_t *calls, uint64_t *reads)
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
    if ((rc = (h->*timer).settle()) != KID_OK) return rc;
    (h->*timer).take(device_ms, calls, reads);
    return check ? kid_hits_check(h) : KID_OK;
}

extern "C" int kid_db_read_hits_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, &KidHitsState::pass, true, device_ms, calls, reads);
}
