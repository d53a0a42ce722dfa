// kid_api_hits.h -- every read's k-mer hits: the scratch of a database's hit passes and kid_db_read_hits*.
// What the other families over the hit pass -- kid_db_read_support* (kid_api_support.h), kid_db_read_fragments*
// (kid_api_fragments.h), kid_db_read_segments* (kid_api_segments.h), kid_db_read_votes* (kid_api_votes.h), kid_db_read_fragment_votes* (kid_api_fragment_votes.h),
// kid_db_read_segment_votes* (kid_api_segment_votes.h), kid_db_read_loci* (kid_api_loci.h) -- share with kid_db_read_hits* is here once:
// KidSpanTimer, KidFamily and KidFamilyState (a family's id, and its share of the state under that id), KidVoteScratch
// and kid_vote_scratch_bind (the scratch of a vote family's second kernel), kid_hits_state (the scratch, free: the
// timers a family settles), kid_hits_scan (the three-kernel exclusive scan), KidOpenBatch and kid_hits_open_* (a
// host-buffer batch checked, locked and staged, one function per input form over kid_hits_stage_*), the hit pass into
// the library's own buffers (kid_hits_host_pass), the checks of a CSR output.
#pragma once
#include "kid_api_db.h"
#include "kid_api_mask.h"
#include "kid_hits.hip.h"

// ---------------------------------------------------------------- every read's k-mer hits (kid_hits.hip.h)
// Scratch of the hit pass: grow-only device buffers sized by the largest batch seen, one set per database (calls on
// one kid_db run one after the other: a call first waits for the kernels of the call before).  Per batch: 16 B per
// read (descriptors) + 8 B per read (first tile) + 16 B per tile of 64 windows (mask, first hit) + 8 B per 1024 of
// either (scan totals); the host-buffer forms add a device copy of their inputs and outputs.  kid_db_read_segments* add
// 16 B per tile (valid mask, its scan), 8 B per read (first segment) and 32 B per segment (host forms);
// kid_db_read_segment_votes* the same with 40 B per segment, and 24 B per segment the call can write (the second kernel's list).
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

// The families of calls over the hit pass (the files named on top).  A family's struct (KidSupportCalls, ..) names its id;
// KidHitsState::family[id] is its share of the state, bit kid_settle(id) its timer in the mask of kid_hits_state.
enum KidFamily : int {
    KID_FAM_PASS = -1, // (kid_hits_take_time: the hit pass, which is not a family)
    KID_FAM_SEGMENTS,
    KID_FAM_SEGMENT_VOTES,
    KID_FAM_SUPPORT,
    KID_FAM_FRAGMENTS,
    KID_FAM_VOTES,
    KID_FAM_FRAGMENT_VOTES,
    KID_FAM_LOCI,
    KID_FAM_FRAGMENT_LOCI,
    KID_FAM_COUNT
};
constexpr unsigned kid_settle(KidFamily f) { return 1u << f; }
// What every call waits for beside the pass, whatever its family: the segment and segment-vote kernels read the tiles'
// scratch behind the pass (and the segment-vote kernels the vote family's rows).
constexpr unsigned KID_SETTLE_ALWAYS = kid_settle(KID_FAM_SEGMENTS) | kid_settle(KID_FAM_SEGMENT_VOTES);

struct KidFamilyState {
    KidDevBuf out;      // the host forms' records
    KidSpanTimer timer; // the family's kernels alone, behind the pass
};

// What the second kernel of a vote family works on: the units its first kernel leaves to it (with more than
// KID_VOTE_WAVE_HITS hits) and their number (one word), one row uint32[ntar] per workgroup (num_cu of them), zero between
// calls.  One set per family and kid_db: a family's settle mask names whoever may still be using the set it binds.
struct KidVoteScratch {
    KidDevBuf list, n_list, own_rows;
    KidDevBuf *rows = &own_rows; // (the segment-vote family's: the vote family's, KidHitsState())
};

// What the second kernel of a loci family works on: the units its first kernel leaves to it (uint32 per unit of the
// largest batch) and their number (one word).  One set per family and kid_db.
struct KidLociScratch {
    KidDevBuf list, n_list;
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
    KidSpanTimer pass; // the hit pass of every call, a family's host call's included
    KidFamilyState family[KID_FAM_COUNT];
    // kid_db_read_segments*, kid_db_read_segment_votes* (kid_api_segments.h): per tile the mask of its lanes that hold a
    // k-mer and their scan (the hit pass stores the mask while want_valid is set: the buffer is sized for the batch then),
    // [0] the batch's segments and [1] its valid windows, the host forms' offsets
    KidDevBuf tile_valid, tile_valid_off, seg_ctl, out_seg_offsets;
    bool want_valid = false;
    // kid_db_read_votes* (a list of uint32 per read of the largest batch), kid_db_read_fragment_votes* (the same set once
    // more, of its own: a vote call and a fragment-vote call queued on two streams never share a list or a row; the list
    // holds fragment indexes), kid_db_read_segment_votes* (a list of 24 B per segment the call can write, and the vote
    // family's rows)
    KidVoteScratch vote_big, fragment_vote_big, segment_vote_big;
    // kid_db_read_loci* (kid_api_loci.h, which binds them), kid_db_read_fragment_loci* (the same set once more, of its own; the
    // list holds fragment indexes)
    KidLociScratch loci_big, fragment_loci_big;
    KidDevBuf lowc_plane; // KID_DB_OPT_LOW_COMPLEXITY: the flag plane of a staged block with a line that is split (kid_lowc.hip.h)
    KidHitsState() { segment_vote_big.rows = &vote_big.own_rows; }
    unsigned long long *ctl() const { return ctl_buf.as<unsigned long long>(); }
};
#define KID_HITS_CTL_WORDS 36u

kid_db::~kid_db() {}

// a little slack: batches of a file differ slightly in size
static hipError_t kid_hits_ensure(KidDevBuf &b, uint64_t nbytes) { return b.ensure(nbytes, ((nbytes + nbytes / 8) + 255u) & ~255ull); }

// The units of a batch bound to a vote scratch on `stream`: a list of list_nbytes, the rows grown to num_cu * ntar words
// (the kernels leave them zero: only new ones are zeroed), no unit on the list.
static int kid_vote_scratch_bind(const kid_db *db, KidVoteScratch &s, uint64_t list_nbytes, hipStream_t stream)
{
    const size_t rows_nbytes = (size_t)db->num_cu * (size_t)db->d.ntar * 4u;
    KID_HIP(kid_hits_ensure(s.list, list_nbytes));
    if (!s.n_list.p) KID_HIP(s.n_list.alloc(4));
    if (rows_nbytes > s.rows->cap) {
        KID_HIP(s.rows->alloc(rows_nbytes));
        KID_HIP(hipMemsetAsync(s.rows->p, 0, rows_nbytes, stream));
    }
    KID_HIP(hipMemsetAsync(s.n_list.p, 0, 4, stream));
    return KID_OK;
}

// The scratch, free: the hit pass of the call before and the kernels of KID_SETTLE_ALWAYS are through -- and of the
// kernels that read the pass's CSR alone those that `settle` names: a call waits for the timers its family has always
// waited for, no more (a device-form caller that queues hits -> support on a stream of its own does not block in the
// next kid_db_read_hits_device).
static int kid_hits_state(kid_db *db, unsigned settle, KidHitsState **out)
{
    if (!db->hits) {
        std::unique_ptr<KidHitsState> h(new KidHitsState());
        const size_t nb = KID_HITS_CTL_WORDS * 8 + sizeof(KidRareArgs);
        KID_HIP(h->ctl_buf.alloc(nb));
        KID_HIP(hipMemset(h->ctl(), 0, nb));
        KID_HIP(h->pass.create());
        for (KidFamilyState &f : h->family) KID_HIP(f.timer.create());
        db->hits = std::move(h);
    }
    KidHitsState *h = *out = db->hits.get();
    int rc = h->pass.settle();
    for (unsigned f = 0; f < KID_FAM_COUNT && rc == KID_OK; f++)
        if ((settle | KID_SETTLE_ALWAYS) >> f & 1u) rc = h->family[f].timer.settle();
    return rc;
}

// A batch of a host-buffer form, opened (kid_hits_open_offsets / _fastq below): checked, the database's lock taken and
// held while this lives, the scratch free, the batch staged in it.
struct KidOpenBatch {
    std::unique_lock<std::mutex> lock;
    KidHitsState *h = nullptr;
    KidBatch b{};                        // the staged copy
    const KidFastqRec *d_recs = nullptr; // FASTQ form: its records (b.start and b.stop are outputs of the prepare kernel then)
    uint64_t max_tiles = 0;              // what the tile arrays are sized for (kid_hits_launch)
    uint32_t longest = 0;                // FASTQ form under a mask option: the longest sequence line, for the mask kernels
};

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

// Exclusive scan on `stream` of the values kid_hits_scan_local_kernel<SRC> finds in `src` (0: tiles of a read's
// descriptor, 1: set bits of a tile's mask, 2: the number itself): out[i] = the sum in front of value i, *total = the
// sum of all.  d_n: their number where only the device knows it -- n is then the bound the grids are sized for -- or
// null: n values.  sums: one word per KID_HITS_SCAN_BLOCK values.  A total above `limit` is set to 0 and counted in
// *overflow; clear[n] is zeroed on the way.
template <int SRC>
static void kid_hits_scan(int cu, hipStream_t stream, const void *src, const uint64_t *d_n, uint64_t n, uint64_t *out, uint64_t *sums,
                          uint64_t *total, uint64_t limit = ~0ull, unsigned long long *overflow = nullptr, uint32_t *clear = nullptr)
{
    const uint64_t n_host = d_n ? 0ull : n;
    hipLaunchKernelGGL(kid_hits_scan_local_kernel<SRC>, dim3(kid_grid_for(n, KID_HITS_SCAN_BLOCK, cu * 8)), dim3(256), 0, stream, src, d_n,
                       n_host, out, sums, clear);
    hipLaunchKernelGGL(kid_hits_scan_top_kernel, dim3(1), dim3(1024), 0, stream, sums, d_n, n_host, total, limit, overflow);
    hipLaunchKernelGGL(kid_hits_scan_add_kernel, dim3(kid_grid_for(n, 256, cu * 8)), dim3(256), 0, stream, out, (const uint64_t *)sums, d_n,
                       n_host, (const uint64_t *)total);
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
    kid_hits_scan<0>(cu, stream, desc, nullptr, n, tile_off, h->rsum.as<uint64_t>(), n_tiles, max_tiles, h->ctl() + 35, d_n_kmers);
    const KidHitsTiles a = kid_hits_tiles(h, b);
    const int tile_grid = kid_grid_for(max_tiles, KID_HITS_WG_TILES, cu * 32);
    hipLaunchKernelGGL(kid_hits_count_kernel, dim3(tile_grid), dim3(256), 0, stream, db->d, a, d_n_kmers);
    // hits per tile -> first hit of every tile
    kid_hits_scan<1>(cu, stream, a.tile_mask, n_tiles, max_tiles, tile_hit_off, h->tsum.as<uint64_t>(), n_hits);
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
static int kid_hits_host_pass(kid_db *db, const KidOpenBatch &ob, uint64_t limit, uint64_t *n_hits)
{
    KidHitsState *h = ob.h;
    const uint64_t n = ob.b.n;
    KID_HIP(kid_hits_ensure(h->out_offsets, (n + 1) * 8));
    KID_HIP(kid_hits_ensure(h->out_nk, n * 4));
    uint64_t *d_total = reinterpret_cast<uint64_t *>(h->ctl() + 33);
    int rc = kid_hits_launch(db, h, ob.b, ob.d_recs, ob.max_tiles, h->out_offsets.as<uint64_t>(), h->out_nk.as<uint32_t>(), nullptr, 0, nullptr,
                             0, false);
    if (rc != KID_OK) return rc;
    uint64_t total = 0;
    KID_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, 0));
    KID_HIP(hipStreamSynchronize(0));
    if (total > 0 && total <= limit) {
        KID_HIP(kid_hits_ensure(h->out_hits, total * sizeof(KidHit)));
        if ((rc = kid_hits_launch_fill(db, h, ob.b, ob.d_recs, ob.max_tiles, h->out_hits.as<KidHit>(), total, 0)) != KID_OK) return rc;
    }
    *n_hits = total;
    return h->pass.end(0, n);
}

// the host-buffer forms behind their uploads: the hit pass, the fill if the caller's buffer holds it, downloads
static int kid_hits_host_run(kid_db *db, const KidOpenBatch &ob, uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap,
                             uint64_t *n_hits)
{
    static_assert(sizeof(kid_hit) == sizeof(KidHit), "kid_hit is the device record");
    KidHitsState *h = ob.h;
    const uint64_t n = ob.b.n, limit = hits ? cap : 0;
    uint64_t total = 0;
    int rc = kid_hits_host_pass(db, ob, limit, &total);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpy(hit_offsets, h->out_offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (n_kmers) KID_HIP(hipMemcpy(n_kmers, h->out_nk.p, n * 4, hipMemcpyDeviceToHost));
    if (total > 0 && total <= limit) KID_HIP(hipMemcpy(hits, h->out_hits.p, total * sizeof(KidHit), hipMemcpyDeviceToHost));
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    *n_hits = total;
    return KID_OK;
}

// The host-buffer forms.  kid_hits_stage_*, one per input form: the batch copied into the scratch (synchronous copies on
// stream 0) -> the KidBatch of the copy, the only place that uploads.  kid_hits_open_*, one per input form, in front of
// them: the database's lock, what the host can refuse about the arguments of a batch that has reads, the database's
// device selected, the scratch free (kid_hits_state with the family's `settle`), the batch staged.
static int kid_hits_stage_text(KidHitsState *h, const uint8_t *src, uint64_t nbytes, KidBatch *b, const uint8_t *src2 = nullptr,
                               uint64_t nbytes2 = 0)
{
    KID_HIP(kid_hits_ensure(h->in_bases, kid_text_bytes(nbytes + nbytes2)));
    b->bases = h->in_bases.as<uint8_t>();
    return kid_upload_text(h->in_bases, src, nbytes, 0, src2, nbytes2);
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

// (under KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY the staged text is masked here, in that order, in front of
// the hit pass: the caller's is not touched)
// (text2: a second block that goes right behind the first; the offsets in recs count from the first's first byte)
static int kid_hits_stage_fastq(const kid_db *db, KidHitsState *h, const uint8_t *text, uint64_t text_nbytes, const uint8_t *text2,
                                uint64_t nbytes2, const kid_fastq_rec *recs, uint64_t n_reads, uint32_t longest, KidBatch *b,
                                const KidFastqRec **d_recs)
{
    int rc = kid_hits_stage_text(h, text, text_nbytes, b, text2, nbytes2);
    if (rc != KID_OK) return rc;
    KID_HIP(kid_hits_ensure(h->in_recs, n_reads * sizeof(KidFastqRec)));
    KID_HIP(kid_hits_ensure(h->trim_start, n_reads * 4));
    KID_HIP(kid_hits_ensure(h->trim_stop, n_reads * 4));
    KID_HIP(hipMemcpy(h->in_recs.p, recs, n_reads * sizeof(KidFastqRec), hipMemcpyHostToDevice));
    b->start = h->trim_start.as<int32_t>(); // (outputs of the prepare kernel here)
    b->stop = h->trim_stop.as<int32_t>();
    b->n = n_reads;
    *d_recs = h->in_recs.as<KidFastqRec>();
    if (db->min_base_quality > 0) {
        rc = kid_mask_launch_fastq(db, h->in_bases.as<uint8_t>(), *d_recs, n_reads, longest, db->min_base_quality, nullptr, 0);
        if (rc != KID_OK) return rc;
    }
    if (db->low_complexity > 0)
        return kid_lowc_launch(db, h->in_bases.as<uint8_t>(), text_nbytes + nbytes2, *d_recs, nullptr, n_reads, longest, db->low_complexity,
                               &h->lowc_plane, nullptr, 0);
    return KID_OK;
}

// more_scratch (null: none): what a family sizes for the batch between the state and the staging (kid_segments_size)
typedef int (*KidHitsMoreScratch)(KidHitsState *h, uint64_t max_tiles);

static int kid_hits_open_offsets(KidOpenBatch &ob, kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start,
                                 const int32_t *stop, uint64_t n_reads, unsigned settle, KidHitsMoreScratch more_scratch = nullptr)
{
    ob.lock = std::unique_lock<std::mutex>(db->hits_mu);
    if (!bases || !offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((start == nullptr) != (stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    int64_t max_kmers = 0;
    int rc = kid_check_offsets_batch(offsets, start, stop, n_reads, db->info.k, &max_kmers, KID_HITS_TILE, &ob.max_tiles);
    if (rc == KID_OK) rc = kid_use_device(db->device);
    if (rc == KID_OK) rc = kid_hits_state(db, settle, &ob.h);
    if (rc == KID_OK && more_scratch) rc = more_scratch(ob.h, ob.max_tiles);
    if (rc != KID_OK) return rc;
    return kid_hits_stage_offsets(ob.h, bases, offsets, start, stop, n_reads, &ob.b);
}

// (shift: the bytes of block 1, which block 2 is staged behind; the two together stay below 4 GiB)
static std::vector<kid_fastq_rec> kid_fastq_interleave(const kid_fastq_rec *recs1, const kid_fastq_rec *recs2, uint64_t n, uint32_t shift)
{
    std::vector<kid_fastq_rec> merged(2 * n);
    for (uint64_t i = 0; i < n; i++) {
        merged[2 * i] = recs1[i];
        kid_fastq_rec c = recs2[i];
        c.seq_off += shift;
        c.qual_off += shift;
        merged[2 * i + 1] = c;
    }
    return merged;
}

// One block of n_reads records, or (recs2 given) two blocks of n_reads / 2 each, the mates of n_reads / 2 fragments: they
// are staged as one text, block 2 behind block 1, with one record index in interleaved order (read 2i from block 1,
// read 2i + 1 from block 2 with its offsets shifted), so that one hit pass takes both.  (The lock comes first:
// db->min_base_quality and db->low_complexity, under which a block's lines must be in order.)
static int kid_hits_open_fastq(KidOpenBatch &ob, kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs,
                               uint64_t n_reads, unsigned settle, KidHitsMoreScratch more_scratch = nullptr, const uint8_t *text2 = nullptr,
                               uint64_t nbytes2 = 0, const kid_fastq_rec *recs2 = nullptr)
{
    ob.lock = std::unique_lock<std::mutex>(db->hits_mu);
    const bool masking = db->min_base_quality > 0 || db->low_complexity > 0;
    const uint64_t n_block = recs2 ? n_reads / 2 : n_reads;
    if (!recs2 && (!text || !recs)) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_check_fastq_block(recs, n_block, text_nbytes, KID_HITS_TILE, &ob.max_tiles, masking, &ob.longest, recs2 ? "mate 1, " : nullptr);
    if (rc == KID_OK && recs2) rc = kid_check_fastq_block(recs2, n_block, nbytes2, KID_HITS_TILE, &ob.max_tiles, masking, &ob.longest, "mate 2, ");
    if (rc == KID_OK) rc = kid_use_device(db->device);
    if (rc == KID_OK) rc = kid_hits_state(db, settle, &ob.h);
    if (rc == KID_OK && more_scratch) rc = more_scratch(ob.h, ob.max_tiles);
    if (rc != KID_OK) return rc;
    std::vector<kid_fastq_rec> merged; // (a synchronous copy reads it)
    if (recs2) {
        merged = kid_fastq_interleave(recs, recs2, n_block, (uint32_t)text_nbytes);
        recs = merged.data();
    }
    return kid_hits_stage_fastq(db, ob.h, text, text_nbytes, text2, nbytes2, recs, n_reads, ob.longest, &ob.b, &ob.d_recs);
}

// The CSR outputs of a call -- offsets[n_reads + 1], up to `cap` records (`what`), their number -- as the host forms
// check them, and as a call without reads leaves them, on the host and in device memory (d_n2: a second number).
static int kid_check_csr_out(const kid_db *db, const uint64_t *out_offsets, const void *records, uint64_t cap, const uint64_t *n_out,
                             uint64_t n_reads, const char *what)
{
    if (!db || !out_offsets || !n_out) return kid_fail(KID_ERR_ARG, "null argument");
    const int rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (cap && !records) return kid_fail(KID_ERR_ARG, "cap without a %s buffer", what);
    return KID_OK;
}
static int kid_csr_out_empty(uint64_t *out_offsets, uint64_t *n_out)
{
    out_offsets[0] = 0;
    *n_out = 0;
    return KID_OK;
}
static int kid_csr_out_empty_device(hipStream_t stream, void *d_out_offsets, void *d_n, void *d_n2 = nullptr)
{
    KID_HIP(hipMemsetAsync(d_out_offsets, 0, 8, stream));
    KID_HIP(hipMemsetAsync(d_n, 0, 8, stream));
    if (d_n2) KID_HIP(hipMemsetAsync(d_n2, 0, 8, stream));
    return KID_OK;
}

extern "C" int kid_db_read_hits(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                uint64_t n_reads, uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits)
{
    int rc = kid_check_csr_out(db, hit_offsets, hits, cap, n_hits, n_reads, "hits");
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return kid_csr_out_empty(hit_offsets, n_hits);
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, 0)) != KID_OK) return rc;
    return kid_hits_host_run(db, ob, hit_offsets, n_kmers, hits, cap, n_hits);
}

extern "C" int kid_db_read_hits_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                      uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits)
{
    int rc = kid_check_csr_out(db, hit_offsets, hits, cap, n_hits, n_reads, "hits");
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return kid_csr_out_empty(hit_offsets, n_hits);
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, 0)) != KID_OK) return rc;
    return kid_hits_host_run(db, ob, hit_offsets, n_kmers, hits, cap, n_hits);
}

extern "C" int kid_db_read_hits_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                       const void *d_stop, uint64_t n_reads, void *d_hit_offsets, void *d_n_kmers, void *d_hits,
                                       uint64_t cap, void *d_n_hits, void *stream)
{
    if (!db || !d_hit_offsets || !d_n_hits) return kid_fail(KID_ERR_ARG, "null argument");
    KidBatch b{};
    int rc = kid_check_device_batch(d_bases, d_offsets, d_start, d_stop, n_reads, &b);
    if (rc == KID_OK) rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (cap && !d_hits) return kid_fail(KID_ERR_ARG, "cap without a hits buffer");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_reads == 0) return kid_csr_out_empty_device(st, d_hit_offsets, d_n_hits);
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, 0, &h)) != KID_OK) return rc;
    rc = kid_hits_launch(db, h, b, nullptr, bases_nbytes / KID_HITS_TILE + n_reads, (uint64_t *)d_hit_offsets, (uint32_t *)d_n_kmers, (KidHit *)d_hits, cap,
                         (uint64_t *)d_n_hits, st, true);
    if (rc != KID_OK) return rc;
    return h->pass.end(st, n_reads);
}

// kid_db_read_hits_time and every family's *_time: the timer of the pass or of a family, settled and taken; the pass's
// query reports what the prepare kernels refused since the last query as well
static int kid_hits_take_time(kid_db *db, KidFamily f, double *device_ms, uint64_t *calls, uint64_t *reads)
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
    KidSpanTimer &timer = f == KID_FAM_PASS ? h->pass : h->family[f].timer;
    if ((rc = timer.settle()) != KID_OK) return rc;
    timer.take(device_ms, calls, reads);
    return f == KID_FAM_PASS ? kid_hits_check(h) : KID_OK;
}

extern "C" int kid_db_read_hits_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KID_FAM_PASS, device_ms, calls, reads);
}
