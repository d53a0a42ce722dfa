// kid_api.hip -- C ABI (include/kmer_id_amd.h) over the gfx950 kernels: the one translation unit of the library.
// Here: the sample handle, the pacing of the hit log, kid_launch_classify and the classify entry points -- the launch
// path a counter profile depends on.  The other areas are the kid_api_*.h files included below (kid_api_support.h
// at the end: it counts into a sample; kid_api_fragments.h, kid_api_votes.h, kid_api_fragment_votes.h, kid_api_segments.h,
// kid_api_segment_votes.h, kid_api_loci.h, kid_api_pileup.h, kid_api_depth.h, kid_api_shared.h and kid_api_coverage.h behind it).  Host side only:
// handle bookkeeping and launches; no classification work is done on the CPU.
#include <hip/hip_runtime.h>
#include <memory>
#include <stdint.h>
#include <string.h>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/kmer_id_amd.h"
#include "kid_kernels.hip.h"
#include "kid_build.hip.h"
#include "kid_tile.hip.h"
#include "kid_long.hip.h"
#include "kid_hits.hip.h"
#include "kid_support.hip.h"
#include "kid_segments.hip.h"
#include "kid_mask.hip.h"
#include "kid_lowc.hip.h"
#include "kid_depth.hip.h"
#include "kid_shared.hip.h"
#include "kid_coverage.hip.h"
#include "kid_loci.hip.h"
#include "kid_pileup.hip.h"
#include "kid_api_core.h"
#include "kid_api_db.h"
#include "kid_api_mask.h"
#include "kid_api_hits.h"
#include "kid_api_builder.h"
#include "kid_api_bench.h"

struct kid_sample {
    kid_db *db = nullptr;
    // The streams come first: members go in reverse order, so they outlive the events and buffers used on them.
    KidStream stream;
    KidStream prep_stream; // the prepare kernel of kid_classify_batch_device when the caller promised KID_OPT_INPUTS_READY
    KidStream copy_stream, out_stream; // the host-buffer entry points: see Slot
    KidDevBuf gcount, ucount; // unsigned long long [ntar]
    KidDevBuf stats;          // unsigned long long [32]: [0..7] counters, [8..31] KID_PROFILE phase cycles
    KidDevBuf seen;           // uint32: the bitmap
    uint64_t seen_words = 0;
    KidDevBuf depth;          // uint32 per entry (padded like the bitmap), while KID_OPT_ENTRY_DEPTH is on: kid_api_depth.h
    bool timing = false;
    std::vector<std::pair<KidEvent, KidEvent>> timed; // around each classify launch, while timing is on
    uint64_t timed_batches = 0;
    // ... read off by a query: ms per batch that kid_sample_kernel_times has not reported yet (the latest KID_TIMED_KEEP
    // of them), and the sum of those kid_sample_kernel_time has not
    std::vector<double> timed_ms;
    double timed_ms_unsummed = 0;
    uint32_t batch_seq = 0;
    // Per-batch scratch of the device pipeline (prepare -> classify), grown on demand.  Three sets taken in turn, so
    // that the prepare kernel of batch b + 1 can run (on another stream) while the classify kernels of batch b still
    // read theirs: the descriptors and the device argument block the kernels find them in.  (The read text is not
    // copied: the classify kernels read the caller's ASCII and pack in registers.  Only a batch with very long records
    // gets a packed image, for the long-record kernels.)
    struct Scratch {
        KidDevBuf desc;      // KidReadDesc per read
        KidDevBuf long_list; // KidLongList: very long records of the batch, flagged by the prepare kernel ...
        KidDevBuf long_plan; // KidLongPlan: ... placed by kid_long_plan_kernel (allocated with the first batch that can hold one)
        KidDevBuf rare;      // KidRareArgs: device copy, written in kid_sample_begin (per batch: batch_max, desc, out_final)
        KidEvent ev_prep;    // the prepare kernel (+ pack) of the batch using the set is done
        KidEvent ev_used;    // ... its classify kernels are done: the set may be overwritten (recorded when a pack on another stream asks)
        hipStream_t used_stream = nullptr; // the stream those classify kernels were queued on (the caller's or ours: not owned)
        bool used_recorded = false;        // ev_used was recorded right behind them
        bool used = false;
    };
    static const int NSET = 3;
    Scratch sets[NSET];
    uint32_t next_set = 0;
    bool inputs_ready = false;
    int min_base_quality = 0; // KID_OPT_MIN_BASE_QUALITY: FASTQ blocks have their low-quality bases masked behind the upload (kid_mask.hip.h)
    KidDevBuf masked;         // unsigned long long [2]: bases masked since the last reset, by quality and ([1]) by low complexity
    int low_complexity = 0;   // KID_OPT_LOW_COMPLEXITY: ... and their low-complexity bases behind that (kid_lowc.hip.h)
    int64_t long_kmers = 65536; // records of more k-mers than this take the long-record kernels (KID_OPT_LONG_RECORD_KMERS)
    // fixed-layout batches have no descriptors and no prepare kernel: one argument block of their own, rewritten (a
    // one-thread kernel in stream order) only when a launch differs from what the block holds
    KidDevBuf rare_fixed; // KidRareArgs
    struct { uint32_t *out_final = nullptr; uint64_t read0 = 0; uint32_t fixed_len = 0; int32_t fixed_nk = 0; bool valid = false; } fixed_held;
    uint64_t dev_clock_batches = 0; // batches since kid_sample_kernel_time_device was last asked
    // the hit log (kid_seenlog.hip.h): where the resolver leaves the entry ordinals of its hits, and the
    // scratch of the pass that turns them into bits of `seen` (all uint32; none of it without a log)
    KidDevBuf seen_log, seen_log_tail, seen_sorted, log_counts, log_bin_total;
    uint32_t seen_log_cap = 0, log_nbins = 0;
    KidMappedHost log_host_total; // [0] log places per 1024 reads as of the last pass, [+8] "log off", written by the device
    bool log_dirty = false;            // something may have been logged since the last pass
    bool log_off = false;              // a pass has found this sample's reads to hit so often that atomics from the resolver are cheaper
    uint32_t passes_done = 0;
    uint32_t launches_since_apply = 0;
    uint64_t reads_since_apply = 0;
    double log_entries_per_read = 4.0; // pace of the passes: a guess until the first pass has reported
    uint64_t reads_of_last_pass = 0;
    // very long records: one word per k-mer position for the hits, one byte per tile of 256 positions ("holds a hit").
    // They grow together: long_tiles holds 16 bytes more than the tiles it is said to have.
    KidDevBuf long_hits, long_tiles;
    bool ended = false; // kid_sample_end* has read the counters and no reset has followed: classify calls and tallies are refused
    uint64_t reads_submitted = 0; // since the last reset: checked against the device's count when results are read
    // KID_OPT_LINE_DIGEST: 0 the pair and duo loops read table headers, 1 the digest plane, 2 (default) the plane until a
    // pass over the hit log gives the log up (log_off below: more than 8 log places per read), then headers until the
    // next reset.  The digest kernels are the faster ones well beyond that rate (profiles/digest/crossover.txt), but
    // the log's rate is the only signal the host has, and it ends there.
    int line_digest = 2;
    uint64_t kernel_variants = 0; // since the last reset: one bit per kid_classify_kernel instantiation launched (kid_sample_kernel_variants)
    // the scratch below is one set per sample: batches on different streams are ordered behind each other
    hipStream_t last_stream = nullptr; // (the caller's or ours: not owned)
    bool has_last_stream = false;
    KidEvent order_ev;
    // Staging for the host-buffer entry points: a ring of slots so that the upload of batch b + 1 (copy stream) and
    // the download of batch b - 1's results (result stream) run beside the kernels of batch b (the sample's stream).
    struct Slot {
        KidDevBuf bases;
        KidDevBuf offsets, start, stop, out; // per read: uint64 (one more), int32, int32, uint32
        KidDevBuf recs; // KidFastqRec: kid_classify_fastq_async, where the host found the lines of the block's records
        KidDevBuf lowc_plane; // KID_OPT_LOW_COMPLEXITY: the flag plane of a block with a line that is split (kid_lowc.hip.h)
        KidEvent ev_h2d, ev_done, ev_out;
        std::vector<uint64_t> rel; // offsets rebased to the slot (alive until the copy has been issued AND done)
        uint64_t ticket = 0;
        bool busy = false;
    };
    static const int NSLOT = 3;
    Slot slots[NSLOT];
    uint64_t next_ticket = 1;

    unsigned long long *stats_p() const { return stats.as<unsigned long long>(); }
    volatile unsigned long long *log_rate() const { return static_cast<volatile unsigned long long *>(log_host_total.p); }
    volatile unsigned int *log_off_flag() const { return reinterpret_cast<volatile unsigned int *>(static_cast<char *>(log_host_total.p) + 8); }
};

// ---------------------------------------------------------------- sample
extern "C" void kid_sample_destroy(kid_sample *s)
{
    if (!s) return;
    if (s->db) hipSetDevice(s->db->device); // the owners' destructors free on the current device
    hipDeviceSynchronize(); // nothing of the sample goes while a kernel or a copy may still use it
    delete s;
}

static int kid_seenlog_point(kid_sample *s, hipStream_t stream);
extern "C" int kid_sample_reset(kid_sample *s)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    const size_t nt = (size_t)s->db->info.ntar;
    KID_HIP(hipMemset(s->gcount.p, 0, nt * 8));
    KID_HIP(hipMemset(s->ucount.p, 0, nt * 8));
    KID_HIP(hipMemset(s->stats.p, 0, 256));
    KID_HIP(hipMemset(s->masked.p, 0, 16));
    {   // device-clock stamps of a launch: [30] first workgroup start (min), [31] last end (max); see kid_classify_kernel
        const unsigned long long never = ~0ull;
        KID_HIP(hipMemcpy(s->stats_p() + 30, &never, 8, hipMemcpyHostToDevice));
    }
    s->dev_clock_batches = 0;
    s->reads_submitted = 0;
    s->ended = false;
    s->kernel_variants = 0;
    if (s->seen_log_tail.p) KID_HIP(hipMemset(s->seen_log_tail.p, 0, KID_LOG_SHARDS * 64));
    if (s->seen_log.p) { // (a pass may have taken the log out of the argument blocks: KidLogArgs)
        int rc = kid_seenlog_point(s, nullptr);
        if (rc != KID_OK) return rc;
        *s->log_off_flag() = 0;
        *s->log_rate() = 0;
        s->log_off = false;
        s->passes_done = 0;
        s->log_entries_per_read = 4.0;
    }
    s->log_dirty = false;
    s->launches_since_apply = 0;
    s->reads_since_apply = 0;
    KID_HIP(hipMemset(s->seen.p, 0, s->seen_words * 4));
    if (s->depth.p) KID_HIP(hipMemset(s->depth.p, 0, s->seen_words * 32 * 4));
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

extern "C" int kid_sample_begin(kid_db *db, kid_sample **out)
{
    if (!db || !out) return kid_fail(KID_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    std::unique_ptr<kid_sample, void (*)(kid_sample *)> s(new kid_sample(), kid_sample_destroy);
    s->db = db;
    const size_t nt = (size_t)db->info.ntar;
    s->seen_words = db->seen_bits / 32; // one bit per DB entry, whole 16-byte groups
    KID_HIP(s->gcount.alloc(nt * 8));
    KID_HIP(s->ucount.alloc(nt * 8));
    KID_HIP(s->stats.alloc(256));
    KID_HIP(s->masked.alloc(16));
    KID_HIP(s->seen.alloc(s->seen_words * 4));
    KID_HIP(s->stream.create());
    // the hit log: for the minimizer-localised table (its resolver is the one that logs), bitmaps of up to 1024 pieces
    const uint64_t nbins = (db->seen_bits + (1ull << KID_LOG_BIN_BITS) - 1) >> KID_LOG_BIN_BITS;
    if (db->d.minloc && nbins <= 1024) {
        uint64_t total = db->info.n_entries * 2ull;              // the whole log holds 2 x the entries of the database ...
        if (total < (32ull << 20)) total = 32ull << 20;          // ... at least 32 M (a launch of 1 M pairs with 16 hits per read) ...
        if (total > (128ull << 20)) total = 128ull << 20;        // ... at most 128 M hits = 512 MiB (+ as much to sort them)
        uint64_t cap = (total / KID_LOG_SHARDS) & ~63ull;        // per region
        s->seen_log_cap = (uint32_t)cap;
        s->log_nbins = (uint32_t)nbins;
        KID_HIP(s->seen_log.alloc(cap * KID_LOG_SHARDS * 4));
        KID_HIP(s->seen_sorted.alloc(cap * KID_LOG_SHARDS * 4));
        KID_HIP(s->seen_log_tail.alloc(KID_LOG_SHARDS * 64));
        KID_HIP(s->log_counts.alloc(nbins * KID_LOG_WGS * 4));
        KID_HIP(s->log_bin_total.alloc(nbins * 4));
        KID_HIP(s->log_host_total.alloc(64, hipHostMallocMapped));
        memset(s->log_host_total.p, 0, 64);
    }
    const KidRareArgs ra{s->gcount.as<unsigned long long>(), s->stats_p(), db->d.line_mask, 0u, 0ull, 0ull, 0, 0u, db->d.rows,
                         s->seen.as<uint32_t>(), nullptr, nullptr, s->seen_log.as<uint32_t>(), s->seen_log_tail.as<uint32_t>(),
                         s->seen_log_cap, 0u, db->d.table};
    for (kid_sample::Scratch &sc : s->sets) {
        KID_HIP(sc.rare.alloc(sizeof(ra)));
        KID_HIP(hipMemcpy(sc.rare.p, &ra, sizeof(ra), hipMemcpyHostToDevice));
        KID_HIP(sc.ev_prep.create(hipEventDisableTiming));
        KID_HIP(sc.ev_used.create(hipEventDisableTiming));
    }
    KID_HIP(s->rare_fixed.alloc(sizeof(ra)));
    KID_HIP(hipMemcpy(s->rare_fixed.p, &ra, sizeof(ra), hipMemcpyHostToDevice));
    rc = kid_sample_reset(s.get());
    if (rc != KID_OK) return rc;
    *out = s.release();
    return KID_OK;
}

// The hit log -> bits of `seen` (kid_seenlog_* kernels), on `stream`, behind everything queued there.
static int kid_seenlog_apply(kid_sample *s, hipStream_t stream)
{
    if (!s->seen_log.p || !s->log_dirty) return KID_OK;
    void *dev_total = nullptr;
    KID_HIP(hipHostGetDevicePointer(&dev_total, s->log_host_total.p, 0));
    const KidLogArgs a{s->seen_log.as<uint32_t>(), s->seen_log_tail.as<uint32_t>(), s->seen_log_cap, s->log_nbins,
                       s->log_counts.as<uint32_t>(), s->log_bin_total.as<uint32_t>(), s->seen_sorted.as<uint32_t>(),
                       s->seen.as<uint32_t>(), s->seen_words, (unsigned long long *)dev_total, s->reads_since_apply,
                       {s->sets[0].rare.as<KidRareArgs>(), s->sets[1].rare.as<KidRareArgs>(), s->sets[2].rare.as<KidRareArgs>(),
                        s->rare_fixed.as<KidRareArgs>()},
                       (unsigned int *)((char *)dev_total + 8)};
    static_assert(kid_sample::NSET == 3, "KidLogArgs::blocks");
    const uint32_t nb = s->log_nbins;
    hipLaunchKernelGGL(kid_seenlog_count_kernel, dim3(KID_LOG_WGS), dim3(256), nb * 4, stream, a);
    hipLaunchKernelGGL(kid_seenlog_scan_kernel, dim3(nb), dim3(KID_LOG_WGS), 0, stream, a);
    hipLaunchKernelGGL(kid_seenlog_scatter_kernel, dim3(KID_LOG_WGS), dim3(256), (4 * nb + 1 + KID_LOG_TILE) * 4, stream, a);
    hipLaunchKernelGGL(kid_seenlog_apply_kernel, dim3(nb), dim3(1024), ((1u << (KID_LOG_BIN_BITS - 5)) + nb + 1) * 4, stream, a);
    KID_HIP(hipMemsetAsync(s->seen_log_tail.p, 0, KID_LOG_SHARDS * 64, stream));
    KID_HIP(hipGetLastError());
    s->reads_of_last_pass = s->reads_since_apply;
    s->log_dirty = false;
    s->launches_since_apply = 0;
    s->reads_since_apply = 0;
    s->passes_done++;
    return KID_OK;
}
// ... when somebody wants to read the bitmap: behind everything the sample has queued anywhere (the caller synchronises after it)
static int kid_seenlog_flush(kid_sample *s)
{
    if (!s->seen_log.p || !s->log_dirty) return KID_OK;
    KID_HIP(hipDeviceSynchronize());
    return kid_seenlog_apply(s, s->stream.s);
}
// the log back into every argument block of the sample (a pass may have taken it out: the resolvers then set the bits
// with atomics), in stream order
static int kid_seenlog_point(kid_sample *s, hipStream_t stream)
{
    KidRareArgs *blocks[kid_sample::NSET + 1];
    int nb = 0;
    for (kid_sample::Scratch &sc : s->sets) blocks[nb++] = sc.rare.as<KidRareArgs>();
    blocks[nb++] = s->rare_fixed.as<KidRareArgs>();
    for (int i = 0; i < nb; i++)
        if (blocks[i]) KID_HIP(hipMemcpyAsync(&blocks[i]->seen_log, &s->seen_log.p, sizeof(uint32_t *), hipMemcpyHostToDevice, stream));
    return KID_OK;
}
// before a launch of n_reads reads: run the pass if the log might not hold what the launch adds.  The device reports
// the entries of every pass (mapped host memory, read without waiting: whatever pass has finished by now), from which
// the hits per read of this sample are known; a region that does fill up falls back to atomics, so the pace only
// matters for speed.
static int kid_seenlog_pace(kid_sample *s, uint64_t n_reads, hipStream_t stream)
{
    if (!s->seen_log.p || s->log_off) return KID_OK;
    if (*s->log_off_flag()) { // a pass found more than 8 hits per read and took the log away (KidLogArgs)
        s->log_off = true;
        return KID_OK;
    }
    const unsigned long long rate = *s->log_rate(); // places per 1024 reads | 1 << 63, from the latest pass that has run
    if (rate >> 63) {
        const double r = (double)(rate & ~(1ull << 63)) / 1024.0;
        s->log_entries_per_read = r > 0.01 ? r * 1.1 : 0.011;
    }
    // (A first pass right behind a sample's first launch would tell early what kind of sample it is -- and made every
    // later launch of the metric's workload 3 % slower, profiles/r03/ab_early_pass.txt; the first regular pass comes
    // after 4 M reads.)
    const double room = 0.5 * (double)s->seen_log_cap * KID_LOG_SHARDS;
    if (s->log_dirty && ((double)(s->reads_since_apply + n_reads) * s->log_entries_per_read > room || s->launches_since_apply >= 256)) {
        int rc = kid_seenlog_apply(s, stream);
        if (rc != KID_OK) return rc;
    }
    s->reads_since_apply += n_reads;
    s->launches_since_apply++;
    s->log_dirty = true;
    return KID_OK;
}

// The kernels that count into a sample run one after the other (they share the sample's counters' timing stamps and
// argument blocks): work issued on another stream than the one before is made to wait for it.
static int kid_sample_order_behind(kid_sample *s, hipStream_t stream)
{
    if (s->has_last_stream && s->last_stream != stream) {
        if (!s->order_ev.e) KID_HIP(s->order_ev.create(hipEventDisableTiming));
        KID_HIP(hipEventRecord(s->order_ev.e, s->last_stream));
        KID_HIP(hipStreamWaitEvent(stream, s->order_ev.e, 0));
    }
    s->last_stream = stream;
    s->has_last_stream = true;
    return KID_OK;
}

// a runtime bool as a template argument: f(std::true_type) or f(std::false_type)
template <class F> static inline void kid_lift(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// One batch on `stream`: kid_prepare_kernel (read descriptors, range checks, longest read -- not for fixed-layout
// batches, whose reads need no descriptors) and the instantiation(s) of kid_classify_kernel (512-thread workgroups =
// 8 waves; pair loop / duo loop / general loops -- the ones the batch is not for return at once; the gcount histogram
// lives in LDS when 4 workgroups per CU still fit).  The kernels read the caller's ASCII text directly.
// max_kmers: the largest n_kmers of the batch when the host knows it (then only the kernel the batch is for is
// launched), -1 when only the device does
// long_records: the batch may hold records of more than s->long_kmers k-mers (FASTA contigs): those take the
// long-record kernels; the host does not need to know which they are
// prep_stream: where the prepare kernel runs.  The same as `stream` unless the read text is known to be ready earlier
// than stream order says (host path: the copy stream behind the upload; kid_classify_batch_device under
// KID_OPT_INPUTS_READY: an internal stream) -- then it overlaps with the classify kernels of the batch before.
// fastq: the batch is a block of FASTQ text with the host's line index (kid_classify_fastq_async); b.bases = the text,
// b.start / b.stop = device arrays that RECEIVE what process_qual computes
static int kid_launch_classify(kid_sample *s, const KidBatch &b, uint64_t bases_nbytes, hipStream_t stream, int64_t max_kmers,
                               hipStream_t prep_stream, bool long_records = false, const KidFastqRec *fastq = nullptr)
{
    kid_db *db = s->db;
    if (b.n == 0) return KID_OK;
    if (b.n > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (bases_nbytes >> 48) return kid_fail(KID_ERR_ARG, "a batch of 2^48 bytes or more");
    const bool fixed = b.offsets == nullptr && !fastq; // fixed layout: whole reads of b.fixed_len bases back to back
    const uint32_t long_cut = (long_records && !fastq && s->long_kmers > 0 && s->long_kmers < 0xFFFFFFFFll &&
                               bases_nbytes > (uint64_t)s->long_kmers) ? (uint32_t)s->long_kmers : 0u;
    if (long_cut) max_kmers = -1; // (the host's number counts the hidden records too: the device's does not)
    {
        int rc = kid_sample_order_behind(s, stream);
        if (rc == KID_OK) rc = kid_seenlog_pace(s, b.n, stream);
        if (rc != KID_OK) return rc;
    }
    unsigned long long *const gcount = s->gcount.as<unsigned long long>(), *const stats = s->stats_p();
    uint32_t *const seen = s->seen.as<uint32_t>();
    kid_sample::Scratch *scp = nullptr;
    KidRareArgs *rare = s->rare_fixed.as<KidRareArgs>();
    KidReadDesc *desc = nullptr;
    if (!fixed) {
        kid_sample::Scratch &sc = s->sets[s->next_set++ % kid_sample::NSET];
        scp = &sc;
        rare = sc.rare.as<KidRareArgs>();
        if (b.n * sizeof(KidReadDesc) > sc.desc.cap) KID_HIP(hipDeviceSynchronize()); // (scratch in use is not freed)
        KID_HIP(sc.desc.ensure(b.n * sizeof(KidReadDesc), b.n * sizeof(KidReadDesc)));
        desc = sc.desc.as<KidReadDesc>();
        if (long_cut) {
            if (!sc.long_plan.p) {
                KID_HIP(sc.long_list.alloc(sizeof(KidLongList)));
                // (in front of the prepare kernel that counts into it, on its stream: a hipMemset runs on the null stream,
                //  behind everything the sample's stream holds and not ordered with the non-blocking copy stream at all --
                //  it emptied the list after the prepare kernel of the set's first batch had filled it, and the batch's
                //  long records came back as reads without k-mers)
                KID_HIP(hipMemsetAsync(sc.long_list.p, 0, 16, prep_stream));
                KID_HIP(sc.long_plan.alloc(sizeof(KidLongPlan)));
            }
            // one word per k-mer position of the long records, one flag per 256: as many as the batch has bases (a bound
            // the host knows), at most 128 M (records beyond that stay with the classify kernels)
            const uint64_t want = bases_nbytes < (128ull << 20) ? bases_nbytes : (128ull << 20);
            if (want * 4 > s->long_hits.cap) {
                KID_HIP(hipDeviceSynchronize());
                const uint64_t cap = want + want / 4;
                // (both given up, and long_hits, whose size is what is asked above, allocated last: whichever allocation
                // fails, long_hits is empty afterwards and the next batch comes here again)
                s->long_hits.reset();
                s->long_tiles.reset();
                KID_HIP(s->long_tiles.ensure(cap / 256 + KID_LONG_MAX + 16, cap / 256 + KID_LONG_MAX + 16));
                KID_HIP(s->long_hits.ensure(want * 4, cap * 4));
            }
        }
        // The batch that used this set three batches ago must be through its classify kernels before the set is overwritten.
        // On the stream those kernels ran on that is a matter of stream order; only a different prepare stream needs an
        // event -- recorded behind the set's classify kernels when those ran beside a prepare stream (the host path), else
        // now, behind everything queued on that stream so far (an event per batch, recorded and waited for, kept the GPU idle
        // for ~10 us of every step).
        if (sc.used && sc.used_stream != prep_stream) {
            if (sc.used_recorded || hipEventRecord(sc.ev_used.e, sc.used_stream) == hipSuccess) KID_HIP(hipStreamWaitEvent(prep_stream, sc.ev_used.e, 0));
            else { // (a caller's stream that is gone by now: everything queued on it has run or the device is in error)
                (void)hipGetLastError();
                KID_HIP(hipDeviceSynchronize());
            }
        }
        const bool fuse_rebase = prep_stream == stream;
        if (fastq)
            hipLaunchKernelGGL(kid_prepare_fastq_kernel, dim3(kid_grid_for(b.n, 256, db->num_cu * 8)), dim3(256), 0, prep_stream, b.bases,
                               fastq, b.n, db->info.k, desc, const_cast<int32_t *>(b.start), const_cast<int32_t *>(b.stop),
                               b.out_final, stats, gcount, rare, ++s->batch_seq, fuse_rebase ? 1 : 0);
        else
            hipLaunchKernelGGL(kid_prepare_kernel, dim3(kid_grid_for(b.n, 256, db->num_cu * 8)), dim3(256), 0, prep_stream, b, db->info.k,
                               desc, stats, rare, ++s->batch_seq, long_cut, sc.long_list.as<KidLongList>(), fuse_rebase ? 1 : 0);
        if (prep_stream != stream) {
            KID_HIP(hipEventRecord(sc.ev_prep.e, prep_stream));
            KID_HIP(hipStreamWaitEvent(stream, sc.ev_prep.e, 0));
        }
        if (long_cut) // the flagged records -> their places in the hit array (in classify-stream order, before the kernels)
            hipLaunchKernelGGL(kid_long_plan_kernel, dim3(1), dim3(64), 0, stream, sc.long_list.as<KidLongList>(), sc.long_plan.as<KidLongPlan>(),
                               desc, rare, s->batch_seq, (uint64_t)s->long_hits.cap / 4, (uint64_t)s->long_tiles.cap - 16);
    }
    const int block = 512, wpb = block / 64;
    const uint32_t ntar = (uint32_t)db->info.ntar;
    // the gcount histogram lives in LDS while four workgroups per CU (160 KiB) still fit beside the waves' strips
    // and queues.  Minimizer-localised table: two 16-bit counters per word, so a workgroup must stay below 65536
    // reads per launch -- a larger batch is classified in several launches of the same grid (`span` reads each).
    const bool ml = db->d.minloc != 0;
    // Workgroups per CU in the grid.  Four are resident; the SIMDs serve their oldest waves first, so equal shares
    // finish far apart (45 % .. 100 % of a launch) and a grid of exactly the resident workgroups ends at a falling
    // occupancy.  With 16 per CU the dispatcher hands a new workgroup to a CU whenever one is through: 0.97 instead of
    // 1.02 ms per 2 M reads (profiles/r02/ab_grid_mult.txt).
    const int grid = kid_grid_for(b.n, wpb, db->num_cu * 16);
    const uint32_t hist_words32 = (ntar + 3u) & ~3u, hist_words16 = ((ntar + 1u) / 2u + 3u) & ~3u;
    const uint32_t hist_words = ml ? hist_words16 : hist_words32;
    const uint32_t wave_words = ml ? KidWaveLds<true, 0>::total : KidWaveLds<false, 0>::total, pair_words = KidWaveLds<true, 1>::total; // (the duo loop's are the pair loop's)
    const bool hist = (hist_words + wpb * wave_words) * 4u + 32u <= 40u * 1024u;
    const bool hist_pair = (hist_words16 + wpb * pair_words) * 4u + 32u <= 40u * 1024u;
    uint64_t span = b.n;
    if (ml && (hist || hist_pair)) {
        // reads per launch: < 65536 per workgroup -- and with the tapered shares (KID_TAPER) the workgroups dispatched
        // first take up to 1.7 x the average (+ rounding to whole units per wave)
        const uint64_t per_wg = (uint64_t)(65535u - 2u * (uint32_t)wpb - 64u * (uint32_t)wpb) * (KID_TAPER + 1u) / (2u * KID_TAPER);
        // (the bound assumes the two halves of the grid are equal: an odd grid -- only ever a small one -- gets half of it)
        const uint64_t cap = (uint64_t)grid * ((grid & 1) ? per_wg / 2 : per_wg);
        if (span > cap) span = cap;
    }
    KidSampleDev sd{gcount, seen, stats};
    const bool rows = db->d.rows != nullptr, k30 = db->info.k == 30;
    const int32_t fixed_nk = fixed ? (int32_t)(max_kmers > 0 ? max_kmers : 0) : 0;
    // the minimizer-localised table has three kernels (see kid_classify_kernel).  Kernel 1: pairs of single-group reads
    // (<= 128 k-mers); kernel 2: the two groups of a read (<= 256); kernel 0: the rest, and all reads of the other table
    const bool want_pair = ml && (max_kmers < 0 || max_kmers <= 2 * 64);
    const bool want_duo = ml && (max_kmers < 0 || (max_kmers > 2 * 64 && max_kmers <= 4 * 64));
    const bool want_general = !ml || max_kmers < 0 || max_kmers > 4 * 64;
    // the pair and duo loops on the digest plane (KID_OPT_LINE_DIGEST), where the table has one
    const bool digest = ml && db->d.digest != nullptr && (s->line_digest == 1 || (s->line_digest == 2 && !s->log_off));
    KidEvent ev0, ev1;
    if (s->timing) {
        KID_HIP(ev0.create());
        KID_HIP(ev1.create());
        KID_HIP(hipEventRecord(ev0.e, stream));
    }
    for (uint64_t r0 = 0; r0 < b.n; r0 += span) {
        const uint64_t cnt = b.n - r0 < span ? b.n - r0 : span;
        KidInput pk{b.bases, fixed ? nullptr : desc + r0, b.out_final ? b.out_final + r0 : nullptr, cnt};
        // the kernels find this launch's descriptors (or the fixed layout) and result array in the device argument block
        if (fixed) {
            auto &h = s->fixed_held;
            if (!h.valid || h.out_final != pk.out_final || h.read0 != r0 || h.fixed_len != b.fixed_len || h.fixed_nk != fixed_nk) {
                hipLaunchKernelGGL(kid_rebase_kernel, dim3(1), dim3(64), 0, stream, rare, (const KidReadDesc *)nullptr, pk.out_final,
                                   (unsigned long long)r0, b.fixed_len, fixed_nk, (1ull << 32) | (unsigned long long)fixed_nk);
                h.valid = true; h.out_final = pk.out_final; h.read0 = r0; h.fixed_len = b.fixed_len; h.fixed_nk = fixed_nk;
            }
        } else if (r0 != 0 || prep_stream != stream) { // (the first launch of a batch prepared on this stream: done by kid_prepare_kernel)
            hipLaunchKernelGGL(kid_rebase_kernel, dim3(1), dim3(64), 0, stream, rare, pk.desc, pk.out_final, 0ull, 0u, 0, 0ull);
        }
        // kid_classify_kernel<2, rows, h, ml, k == 30 ? 30 : 0, PK> for the runtime values of the four; PK = 1, 2 exist
        // for the minimizer-localised table alone (the discarded branch keeps the others from being instantiated)
        auto launch = [&](auto pk_mode, bool h) {
            constexpr int PK = decltype(pk_mode)::value;
            kid_lift(rows, [&](auto R) { kid_lift(h, [&](auto H) { kid_lift(ml, [&](auto M) { kid_lift(k30, [&](auto K30) {
                kid_lift(PK != 0 && digest, [&](auto D) {
                if constexpr ((PK == 0 || decltype(M)::value) && (!decltype(D)::value || (PK != 0 && decltype(M)::value))) {
                    constexpr bool r = decltype(R)::value, hh = decltype(H)::value, m = decltype(M)::value, dg = decltype(D)::value;
                    constexpr int KF = decltype(K30)::value ? 30 : 0;
                    const uint32_t hw = hh ? (PK ? hist_words16 : hist_words) : 0u;
                    // (the DIGEST instantiations: bits 48..63, see kid_sample_kernel_variants)
                    s->kernel_variants |= dg ? 1ull << (48 + (PK - 1) * 8 + (r << 2 | hh << 1 | (KF == 30)))
                                             : 1ull << (PK * 16 | r << 3 | hh << 2 | m << 1 | (KF == 30));
                    hipLaunchKernelGGL((kid_classify_kernel<2, r, hh, m, KF, PK, dg>), dim3(grid), dim3(block),
                                       (hw + (size_t)wpb * KidWaveLds<m, PK>::total) * 4 + 32, stream, db->d, pk, sd, hw,
                                       pk.desc, rare);
                }
                });
            }); }); }); });
        };
        if (want_pair) launch(std::integral_constant<int, 1>{}, hist_pair);
        if (want_duo) launch(std::integral_constant<int, 2>{}, hist_pair);
        if (want_general) launch(std::integral_constant<int, 0>{}, hist);
    }
    if (long_cut) {
        // the very long records: every k-mer looked up by a lane of its own, then one workgroup per record folds its hits.
        // (The grids do not depend on how many there are -- only the device knows: without any, the kernels return at once.)
        hipLaunchKernelGGL(kid_long_hits_kernel, dim3((unsigned)db->num_cu * 8u), dim3(256), 0, stream, db->d, b.bases,
                           scp->long_plan.as<KidLongPlan>(), s->long_hits.as<uint32_t>(), s->long_tiles.as<uint8_t>(), seen, stats);
        hipLaunchKernelGGL(kid_long_fold_kernel, dim3(KID_LONG_MAX), dim3(256), 0, stream, db->d, scp->long_plan.as<KidLongPlan>(),
                           s->long_hits.as<uint32_t>(), s->long_tiles.as<uint8_t>(), gcount, b.out_final);
    }
    if (s->timing) {
        KID_HIP(hipEventRecord(ev1.e, stream));
        s->timed.emplace_back(std::move(ev0), std::move(ev1));
        s->timed_batches++;
    }
    s->dev_clock_batches++;
    if (scp) {
        // prepare on a stream of its own (the host path: it runs beside the classify kernels of the batch before): the
        // prepare that overwrites this set three batches on waits for exactly these kernels, not for whatever the classify
        // stream holds by then (profiles/r02/ab_lazy_event.txt)
        scp->used_recorded = prep_stream != stream;
        if (scp->used_recorded) KID_HIP(hipEventRecord(scp->ev_used.e, stream));
        scp->used_stream = stream;
        scp->used = true;
    }
    KID_HIP(hipGetLastError());
    s->reads_submitted += b.n;
    return KID_OK;
}

static int kid_depth_set_option(kid_sample *s, int value); // kid_api_depth.h
extern "C" int kid_sample_set_option(kid_sample *s, int option, int value)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    switch (option) {
    case KID_OPT_INPUTS_READY: s->inputs_ready = value != 0; return KID_OK;
    case KID_OPT_LONG_RECORD_KMERS:
        if (value < 0) return kid_fail(KID_ERR_ARG, "KID_OPT_LONG_RECORD_KMERS: negative threshold");
        s->long_kmers = value;
        return KID_OK;
    case KID_OPT_MIN_BASE_QUALITY: {
        int rc = kid_mask_check_q(value);
        if (rc == KID_OK) s->min_base_quality = value;
        return rc;
    }
    case KID_OPT_ENTRY_DEPTH: return kid_depth_set_option(s, value);
    case KID_OPT_LOW_COMPLEXITY: {
        int rc = kid_lowc_check_t(value);
        if (rc == KID_OK) s->low_complexity = value;
        return rc;
    }
    case KID_OPT_LINE_DIGEST:
        if (value < 0 || value > 2) return kid_fail(KID_ERR_ARG, "KID_OPT_LINE_DIGEST: the value is 0, 1 or 2, not %d", value);
        s->line_digest = value;
        return KID_OK;
    default: return kid_fail(KID_ERR_ARG, "unknown option %d", option);
    }
}

// kid_sample_end* has read the counters: nothing more is counted into the sample until kid_sample_reset (KID_ERR_STATE)
static int kid_sample_check_open(const kid_sample *s)
{
    if (s->ended) return kid_fail(KID_ERR_STATE, "classify after kid_sample_end without kid_sample_reset");
    return KID_OK;
}

// pack + prepare stream of the *_device entry points
static int kid_prep_stream_for(kid_sample *s, hipStream_t stream, hipStream_t *out)
{
    *out = stream;
    if (!s->inputs_ready) return KID_OK;
    if (!s->prep_stream.s) KID_HIP(s->prep_stream.create(hipStreamNonBlocking));
    *out = s->prep_stream.s;
    return KID_OK;
}

extern "C" int kid_sample_kernel_variants(kid_sample *s, uint64_t *mask)
{
    if (!s || !mask) return kid_fail(KID_ERR_ARG, "null argument");
    *mask = s->kernel_variants;
    return KID_OK;
}

extern "C" int kid_sample_log_state(kid_sample *s, uint32_t *passes, int *has_log, int *logging)
{
    if (!s || !passes || !has_log || !logging) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize()); // every pass queued so far has run: the flag below is the device's last word
    *passes = s->passes_done;
    *has_log = s->seen_log.p != nullptr;
    *logging = *has_log && *s->log_off_flag() == 0; // (not s->log_off: the host learns of a switch only at its next launch)
    return KID_OK;
}

extern "C" int kid_sample_set_timing(kid_sample *s, int enabled)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    s->timing = enabled != 0;
    return KID_OK;
}

// the event pairs recorded so far -> milliseconds, for both queries below (synchronises)
static int kid_timed_read(kid_sample *s)
{
    static const size_t KID_TIMED_KEEP = 1u << 16;
    KID_HIP(hipDeviceSynchronize());
    for (auto &ev : s->timed) {
        float ms = 0;
        KID_HIP(hipEventElapsedTime(&ms, ev.first.e, ev.second.e));
        s->timed_ms.push_back(ms);
        s->timed_ms_unsummed += ms;
    }
    s->timed.clear();
    if (s->timed_ms.size() > KID_TIMED_KEEP) s->timed_ms.erase(s->timed_ms.begin(), s->timed_ms.end() - KID_TIMED_KEEP);
    return KID_OK;
}

extern "C" int kid_sample_kernel_time(kid_sample *s, double *total_ms, uint64_t *launches)
{
    if (!s || !total_ms || !launches) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc == KID_OK) rc = kid_timed_read(s);
    if (rc != KID_OK) return rc;
    *total_ms = s->timed_ms_unsummed;
    *launches = s->timed_batches; // batches: the kernels of one batch count as one launch
    s->timed_ms_unsummed = 0;
    s->timed_batches = 0;
    return KID_OK;
}

extern "C" int kid_sample_kernel_times(kid_sample *s, double *ms, uint64_t cap, uint64_t *n)
{
    if (!s || !n || (cap && !ms)) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc == KID_OK) rc = kid_timed_read(s);
    if (rc != KID_OK) return rc;
    *n = s->timed_ms.size();
    for (uint64_t i = 0; i < cap && i < *n; i++) ms[i] = s->timed_ms[i];
    s->timed_ms.clear();
    return KID_OK;
}

extern "C" int kid_sample_kernel_time_device(kid_sample *s, double *total_ms, uint64_t *launches)
{
    if (!s || !total_ms || !launches) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    unsigned long long st[32];
    KID_HIP(hipMemcpy(st, s->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    const unsigned long long ticks = st[6]; // banked by the last workgroup of every launch ([7]: launches)
    const unsigned long long zero2[2] = {0, 0};
    KID_HIP(hipMemcpy(s->stats_p() + 6, zero2, 16, hipMemcpyHostToDevice));
    *total_ms = (double)ticks / 1e5; // s_memrealtime: 100 MHz
    *launches = s->dev_clock_batches; // batches, like kid_sample_kernel_time (a large batch is several launches)
    s->dev_clock_batches = 0;
    return KID_OK;
}

extern "C" int kid_classify_batch_device(kid_sample *s, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets,
                                         const void *d_start, const void *d_stop, uint64_t n_reads, void *d_out_final_targ,
                                         void *stream)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null argument");
    KidBatch b{};
    int rc = kid_check_device_batch(d_bases, d_offsets, d_start, d_stop, n_reads, &b);
    if (rc == KID_OK) rc = kid_sample_check_open(s);
    if (rc == KID_OK) rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    b.out_final = (uint32_t *)d_out_final_targ;
    hipStream_t prep;
    rc = kid_prep_stream_for(s, (hipStream_t)stream, &prep);
    if (rc != KID_OK) return rc;
    return kid_launch_classify(s, b, bases_nbytes, (hipStream_t)stream, -1, prep, /*long_records=*/true);
}

extern "C" int kid_classify_fixed_device(kid_sample *s, const void *d_bases, uint32_t read_len, uint64_t n_reads,
                                         void *d_out_final_targ, void *stream)
{
    if (!s || (n_reads && !d_bases)) return kid_fail(KID_ERR_ARG, "null argument");
    if (((uintptr_t)d_bases & 15u) != 0) return kid_fail(KID_ERR_ARG, "d_bases must be 16-byte aligned");
    if (read_len == 0 || read_len > 0x7FFFFFFFu) return kid_fail(KID_ERR_ARG, "read_len out of range");
    int rc = kid_sample_check_open(s);
    if (rc == KID_OK) rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KidBatch b{};
    b.bases = (const uint8_t *)d_bases;
    b.out_final = (uint32_t *)d_out_final_targ;
    b.n = n_reads;
    b.fixed_len = read_len;
    const int64_t nk = (int64_t)read_len - s->db->info.k + 1;
    hipStream_t prep;
    rc = kid_prep_stream_for(s, (hipStream_t)stream, &prep);
    if (rc != KID_OK) return rc;
    return kid_launch_classify(s, b, n_reads * (uint64_t)read_len, (hipStream_t)stream, nk > 0 ? nk : 0, prep);
}

// ---- host buffers: asynchronous slot pipeline -------------------------------------------------------------------
// the slot of the next ticket, free, with room for n_reads reads in nbytes of text
static int kid_slot_acquire(kid_sample *s, uint64_t n_reads, uint64_t nbytes, kid_sample::Slot **out)
{
    if (!s->copy_stream.s) KID_HIP(s->copy_stream.create(hipStreamNonBlocking));
    if (!s->out_stream.s) KID_HIP(s->out_stream.create(hipStreamNonBlocking));
    kid_sample::Slot &sl = s->slots[s->next_ticket % kid_sample::NSLOT];
    if (!sl.ev_out.e) {
        KID_HIP(sl.ev_h2d.create(hipEventDisableTiming));
        KID_HIP(sl.ev_done.create(hipEventDisableTiming));
        KID_HIP(sl.ev_out.create(hipEventDisableTiming));
    }
    if (sl.busy) { // the batch that used this slot three tickets ago
        KID_HIP(hipEventSynchronize(sl.ev_out.e));
        sl.busy = false;
    }
    // a little slack: batches of a file differ slightly in size
    const uint64_t need = kid_text_bytes(nbytes), cap = n_reads + n_reads / 8;
    KID_HIP(sl.bases.ensure(need, need + need / 8));
    KID_HIP(sl.offsets.ensure((n_reads + 1) * 8, (cap + 1) * 8));
    KID_HIP(sl.start.ensure(n_reads * 4, cap * 4));
    KID_HIP(sl.stop.ensure(n_reads * 4, cap * 4));
    KID_HIP(sl.out.ensure(n_reads * 4, cap * 4));
    *out = &sl;
    return KID_OK;
}

// upload issued on the copy stream -> kernels on the sample's stream -> results on the result stream
// (fastq, out_start, out_stop: a FASTQ block, whose trimmed ranges go back to the host with the results)
static int kid_slot_submit(kid_sample *s, kid_sample::Slot &sl, const KidBatch &b, uint64_t nbytes, int64_t max_kmers,
                           uint32_t *out_final_targ, uint64_t *ticket, bool long_records = false,
                           const KidFastqRec *fastq = nullptr, int32_t *out_start = nullptr, int32_t *out_stop = nullptr)
{
    // the prepare kernel follows the upload on the copy stream (beside the classify kernels of the batch before); the
    // classify kernels wait for it on the sample's stream
    KID_HIP(hipEventRecord(sl.ev_h2d.e, s->copy_stream.s));
    // (a fixed-layout batch has no prepare kernel on the copy stream for the classify kernels to wait for: they wait for the upload itself)
    if (!b.offsets && !fastq) KID_HIP(hipStreamWaitEvent(s->stream.s, sl.ev_h2d.e, 0));
    int rc = kid_launch_classify(s, b, nbytes, s->stream.s, max_kmers, s->copy_stream.s, long_records, fastq);
    if (rc != KID_OK) return rc;
    KID_HIP(hipEventRecord(sl.ev_done.e, s->stream.s));
    if (out_final_targ || fastq) {
        hipStream_t os = s->out_stream.s;
        KID_HIP(hipStreamWaitEvent(os, sl.ev_done.e, 0));
        if (out_final_targ) KID_HIP(hipMemcpyAsync(out_final_targ, sl.out.p, b.n * 4, hipMemcpyDeviceToHost, os));
        if (fastq) {
            KID_HIP(hipMemcpyAsync(out_start, sl.start.p, b.n * 4, hipMemcpyDeviceToHost, os));
            KID_HIP(hipMemcpyAsync(out_stop, sl.stop.p, b.n * 4, hipMemcpyDeviceToHost, os));
        }
        KID_HIP(hipEventRecord(sl.ev_out.e, os));
    } else {
        KID_HIP(hipEventRecord(sl.ev_out.e, s->stream.s));
    }
    sl.busy = true;
    sl.ticket = s->next_ticket++;
    if (ticket) *ticket = sl.ticket;
    return KID_OK;
}

extern "C" int kid_classify_batch_async(kid_sample *s, const uint8_t *bases, const uint64_t *offsets, const int32_t *start,
                                        const int32_t *stop, uint64_t n_reads, uint32_t *out_final_targ, uint64_t *ticket)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    if (ticket) *ticket = 0;
    if (n_reads == 0) return KID_OK;
    if (!bases || !offsets) return kid_fail(KID_ERR_ARG, "null argument");
    if ((start == nullptr) != (stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    int64_t max_kmers = 0;
    int rc = kid_sample_check_open(s);
    if (rc != KID_OK) return rc;
    rc = kid_check_offsets_batch(offsets, start, stop, n_reads, s->db->info.k, &max_kmers, 0, nullptr);
    if (rc != KID_OK) return rc;
    // A record of more than s->long_kmers k-mers is a long record (a FASTA contig, kmer_read_vf6.cpp:803-861): the classify
    // kernels would give it to one wave; the launch sorts those out on the device (kid_long_*).
    const bool long_records = s->long_kmers > 0 && max_kmers > s->long_kmers;
    rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    kid_sample::Slot *slp = nullptr;
    rc = kid_slot_acquire(s, n_reads, nbytes, &slp);
    if (rc != KID_OK) return rc;
    kid_sample::Slot &sl = *slp;
    hipStream_t cs = s->copy_stream.s;
    rc = kid_upload_text(sl.bases, bases + base0, nbytes, cs);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpyAsync(sl.offsets.p, kid_rebased_offsets(offsets, n_reads, sl.rel), (n_reads + 1) * 8, hipMemcpyHostToDevice, cs));
    if (start) {
        KID_HIP(hipMemcpyAsync(sl.start.p, start, n_reads * 4, hipMemcpyHostToDevice, cs));
        KID_HIP(hipMemcpyAsync(sl.stop.p, stop, n_reads * 4, hipMemcpyHostToDevice, cs));
    }
    KidBatch b{};
    b.bases = sl.bases.as<uint8_t>();
    b.offsets = sl.offsets.as<uint64_t>();
    b.start = start ? sl.start.as<int32_t>() : nullptr;
    b.stop = start ? sl.stop.as<int32_t>() : nullptr;
    b.out_final = sl.out.as<uint32_t>();
    b.n = n_reads;
    return kid_slot_submit(s, sl, b, nbytes, max_kmers, out_final_targ, ticket, long_records);
}

extern "C" int kid_classify_fixed_async(kid_sample *s, const uint8_t *bases, uint32_t read_len, uint64_t n_reads,
                                        uint32_t *out_final_targ, uint64_t *ticket)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    if (ticket) *ticket = 0;
    if (n_reads == 0) return KID_OK;
    if (!bases) return kid_fail(KID_ERR_ARG, "null argument");
    if (read_len == 0 || read_len > 0x7FFFFFFFu) return kid_fail(KID_ERR_ARG, "read_len out of range");
    int rc = kid_sample_check_open(s);
    if (rc == KID_OK) rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    const uint64_t nbytes = n_reads * (uint64_t)read_len;
    kid_sample::Slot *slp = nullptr;
    rc = kid_slot_acquire(s, n_reads, nbytes, &slp);
    if (rc != KID_OK) return rc;
    kid_sample::Slot &sl = *slp;
    rc = kid_upload_text(sl.bases, bases, nbytes, s->copy_stream.s);
    if (rc != KID_OK) return rc;
    KidBatch b{};
    b.bases = sl.bases.as<uint8_t>();
    b.out_final = sl.out.as<uint32_t>();
    b.n = n_reads;
    b.fixed_len = read_len;
    const int64_t nk = (int64_t)read_len - s->db->info.k + 1;
    return kid_slot_submit(s, sl, b, nbytes, nk > 0 ? nk : 0, out_final_targ, ticket);
}

// A block of FASTQ text whose lines the caller has found: quality trimming (process_qual), the ">= k" test and
// process_read all happen on the GPU; the host's share of process_fqgz (newkmer_10nx.cpp:762-816) is inflate + memchr.
extern "C" int kid_classify_fastq_async(kid_sample *s, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs,
                                        uint64_t n_reads, uint32_t *out_final_targ, int32_t *out_start, int32_t *out_stop,
                                        uint64_t *ticket)
{
    static_assert(sizeof(kid_fastq_rec) == sizeof(KidFastqRec), "kid_fastq_rec is the device record");
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    if (ticket) *ticket = 0;
    if (n_reads == 0) return KID_OK;
    if (!text || !recs || !out_start || !out_stop) return kid_fail(KID_ERR_ARG, "null argument");
    const int mask_q = s->min_base_quality, mask_t = s->low_complexity;
    uint32_t longest = 0;
    int rc = kid_sample_check_open(s);
    if (rc != KID_OK) return rc;
    rc = kid_check_fastq_block(recs, n_reads, text_nbytes, 0, nullptr, mask_q > 0 || mask_t > 0, &longest);
    if (rc != KID_OK) return rc;
    rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    kid_sample::Slot *slp = nullptr;
    rc = kid_slot_acquire(s, n_reads, text_nbytes, &slp);
    if (rc != KID_OK) return rc;
    kid_sample::Slot &sl = *slp;
    const uint64_t cap = n_reads + n_reads / 8;
    KID_HIP(sl.recs.ensure(n_reads * sizeof(KidFastqRec), cap * sizeof(KidFastqRec)));
    hipStream_t cs = s->copy_stream.s;
    rc = kid_upload_text(sl.bases, text, text_nbytes, cs);
    if (rc != KID_OK) return rc;
    KID_HIP(hipMemcpyAsync(sl.recs.p, recs, n_reads * sizeof(KidFastqRec), hipMemcpyHostToDevice, cs));
    // low-quality bases -> 'N' in the slot's copy of the text: on the copy stream, behind the upload and in front of the
    // prepare kernel, whose event the batch's classify kernels wait for (the prepare kernel reads quality bytes alone,
    // which the mask kernel does not write)
    if (mask_q > 0) {
        rc = kid_mask_launch_fastq(s->db, sl.bases.as<uint8_t>(), sl.recs.as<KidFastqRec>(), n_reads, longest, mask_q,
                                   s->masked.as<unsigned long long>(), cs);
        if (rc != KID_OK) return rc;
    }
    // low-complexity bases -> 'N' behind that, on the text the quality mask left, under the same event
    if (mask_t > 0) {
        rc = kid_lowc_launch(s->db, sl.bases.as<uint8_t>(), text_nbytes, sl.recs.as<KidFastqRec>(), nullptr, n_reads, longest, mask_t,
                             &sl.lowc_plane, s->masked.as<unsigned long long>() + 1, cs);
        if (rc != KID_OK) return rc;
    }
    KidBatch b{};
    b.bases = sl.bases.as<uint8_t>();
    b.start = sl.start.as<int32_t>(); // (outputs of the prepare kernel here)
    b.stop = sl.stop.as<int32_t>();
    b.out_final = sl.out.as<uint32_t>();
    b.n = n_reads;
    return kid_slot_submit(s, sl, b, text_nbytes, -1, out_final_targ, ticket, false, sl.recs.as<KidFastqRec>(), out_start, out_stop);
}

extern "C" int kid_classify_wait(kid_sample *s, uint64_t ticket)
{
    if (!s) return kid_fail(KID_ERR_ARG, "null sample");
    if (ticket == 0) return KID_OK; // an empty batch
    if (ticket >= s->next_ticket) return kid_fail(KID_ERR_ARG, "ticket %llu has not been issued", (unsigned long long)ticket);
    kid_sample::Slot &sl = s->slots[ticket % kid_sample::NSLOT];
    if (sl.ticket != ticket || !sl.busy) return KID_OK; // its slot has been waited for (and maybe reused) already
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipEventSynchronize(sl.ev_out.e));
    sl.busy = false;
    return KID_OK;
}

extern "C" int kid_classify_batch(kid_sample *s, const uint8_t *bases, const uint64_t *offsets, const int32_t *start,
                                  const int32_t *stop, uint64_t n_reads, uint32_t *out_final_targ)
{
    uint64_t ticket = 0;
    int rc = kid_classify_batch_async(s, bases, offsets, start, stop, n_reads, out_final_targ, &ticket);
    if (rc != KID_OK) return rc;
    return kid_classify_wait(s, ticket);
}

// ---------------------------------------------------------------- results
static int kid_check_errors(kid_sample *s)
{
    unsigned long long st[9];
    KID_HIP(hipMemcpy(st, s->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st[4] != 0)
        return kid_fail(KID_ERR_ARG, "%llu reads had [start,stop] outside the read (string::at would throw)", st[4]);
    if (st[8] != 0)
        return kid_fail(KID_ERR_FORMAT, "%llu FASTQ records have a quality line shorter than the sequence (qual.at() throws in the reference)", st[8]);
    // every read handed over was classified by exactly one of the kernels (they pick themselves by the batch's
    // longest read: a disagreement with the host's choice would show here, not as silently missing reads)
    if (st[0] != s->reads_submitted)
        return kid_fail(KID_ERR_STATE, "%llu reads classified, %llu submitted", st[0], (unsigned long long)s->reads_submitted);
    return KID_OK;
}

extern "C" int kid_sample_gcount(kid_sample *s, int64_t *gcount)
{
    if (!s || !gcount) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(gcount, s->gcount.p, (size_t)s->db->info.ntar * 8, hipMemcpyDeviceToHost));
    return kid_check_errors(s);
}

extern "C" int kid_sample_ucount_range(kid_sample *s, uint64_t slot_begin, uint64_t slot_end, int64_t *ucount)
{
    if (!s || !ucount) return kid_fail(KID_ERR_ARG, "null argument");
    if (slot_begin > slot_end || slot_end > s->seen_words * 32 || (slot_begin & 127) || (slot_end & 127))
        return kid_fail(KID_ERR_ARG, "bit range must be 128-aligned and inside the bitmap");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    rc = kid_seenlog_flush(s);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    const size_t nt = (size_t)s->db->info.ntar;
    KID_HIP(hipMemset(s->ucount.p, 0, nt * 8));
    const uint64_t w0 = slot_begin / 32, w1 = slot_end / 32;
    if (w1 > w0) {
        const uint32_t ntar = (uint32_t)s->db->info.ntar;
        const int ugrid = kid_grid_for((w1 - w0) / 4, 512, s->db->num_cu * 4);
        if (ntar * 4u <= 64u * 1024u)
            hipLaunchKernelGGL((kid_ucount_kernel<true>), dim3(ugrid), dim3(512), ntar * 4u, 0, s->seen.as<uint32_t>(), w0, w1,
                               s->db->ord_target.as<uint32_t>(), s->ucount.as<unsigned long long>(), ntar);
        else
            hipLaunchKernelGGL((kid_ucount_kernel<false>), dim3(ugrid), dim3(512), 0, 0, s->seen.as<uint32_t>(), w0, w1,
                               s->db->ord_target.as<uint32_t>(), s->ucount.as<unsigned long long>(), ntar);
        KID_HIP(hipGetLastError());
    }
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(ucount, s->ucount.p, nt * 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_end(kid_sample *s, int64_t *gcount, int64_t *ucount)
{
    if (!s || !gcount || !ucount) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_sample_gcount(s, gcount);
    if (rc != KID_OK) return rc;
    rc = kid_sample_ucount_range(s, 0, s->seen_words * 32, ucount);
    if (rc == KID_OK) s->ended = true;
    return rc;
}

// The counters of ONE sample of the input whose batches were dealt out over n kid_sample objects -- one per GPU, each
// on its own replica of the database (kid_db_replicate, or kid_db_build from the same entries).  gcount adds; ucount is
// |distinct DB k-mers hit|: the seen-bitmaps (one bit per DB entry, the same numbering on every replica) are copied
// peer to peer into samples[0]'s GPU, OR-ed there and counted once.  This is the merge of the reference's globals
// (newkmer_10nx.cpp:61-64) over the shards; the process-per-GPU form of it over RCCL is kmer_id_amd/dist.py.
// samples[0]'s bitmap holds the union afterwards.
extern "C" int kid_sample_end_merged(kid_sample **samples, int n, int64_t *gcount, int64_t *ucount)
{
    if (!samples || n < 1 || !gcount || !ucount) return kid_fail(KID_ERR_ARG, "bad argument");
    for (int i = 0; i < n; i++) {
        if (!samples[i]) return kid_fail(KID_ERR_ARG, "samples[%d] is null", i);
        if (samples[i]->seen_words != samples[0]->seen_words || samples[i]->db->info.ntar != samples[0]->db->info.ntar ||
            samples[i]->db->info.n_entries != samples[0]->db->info.n_entries)
            return kid_fail(KID_ERR_ARG, "samples[%d] belongs to a database built from other entries", i);
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++)
            if (samples[i] == samples[j]) return kid_fail(KID_ERR_ARG, "samples[%d] and samples[%d] are the same sample (its reads would be counted twice)", j, i);
    kid_sample *s0 = samples[0];
    const size_t nt = (size_t)s0->db->info.ntar;
    int rc = kid_sample_gcount(s0, gcount);
    if (rc != KID_OK) return rc;
    if (n > 1) {
        std::vector<int64_t> g(nt);
        KidDevBuf tmp;
        rc = kid_use_device(s0->db->device);
        if (rc != KID_OK) return rc;
        const size_t nbytes = (size_t)s0->seen_words * 4;
        KID_HIP(tmp.alloc(nbytes));
        for (int i = 1; i < n; i++) {
            rc = kid_use_device(samples[i]->db->device);
            if (rc != KID_OK) return rc;
            rc = kid_seenlog_flush(samples[i]); // its bitmap is read below
            if (rc != KID_OK) return rc;
            rc = kid_sample_gcount(samples[i], g.data()); // (synchronises samples[i]'s device)
            if (rc != KID_OK) return rc;
            for (size_t t = 0; t < nt; t++) gcount[t] += g[t];
            rc = kid_use_device(s0->db->device);
            if (rc != KID_OK) return rc;
            if (samples[i]->db->device == s0->db->device) KID_HIP(hipMemcpy(tmp.p, samples[i]->seen.p, nbytes, hipMemcpyDeviceToDevice));
            else KID_HIP(hipMemcpyPeer(tmp.p, s0->db->device, samples[i]->seen.p, samples[i]->db->device, nbytes));
            rc = kid_sample_seen_or(s0, 0, nbytes, tmp.p, 1);
            if (rc != KID_OK) return rc;
        }
    }
    rc = kid_sample_ucount_range(s0, 0, s0->seen_words * 32, ucount);
    if (rc == KID_OK)
        for (int i = 0; i < n; i++) samples[i]->ended = true;
    return rc;
}

extern "C" int kid_sample_stats(kid_sample *s, uint64_t out[4])
{
    if (!s || !out) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    unsigned long long st[8];
    KID_HIP(hipMemcpy(st, s->stats.p, 64, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) out[i] = st[i];
    return KID_OK;
}

extern "C" int kid_sample_masked_bases(kid_sample *s, uint64_t *out)
{
    if (!s || !out) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out, s->masked.p, 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_lowc_bases(kid_sample *s, uint64_t *out)
{
    if (!s || !out) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out, s->masked.as<uint64_t>() + 1, 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_seen_bytes(const kid_sample *s, uint64_t *nbytes)
{
    if (!s || !nbytes) return kid_fail(KID_ERR_ARG, "null argument");
    *nbytes = s->seen_words * 4;
    return KID_OK;
}

extern "C" int kid_sample_seen_export(kid_sample *s, uint64_t byte_off, uint64_t nbytes, void *dst, int dst_on_device)
{
    if (!s || (nbytes && !dst)) return kid_fail(KID_ERR_ARG, "null argument");
    if (byte_off + nbytes > s->seen_words * 4) return kid_fail(KID_ERR_ARG, "range outside the bitmap");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    rc = kid_seenlog_flush(s);
    if (rc != KID_OK) return rc;
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(dst, s->seen.as<uint8_t>() + byte_off, nbytes, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_sample_seen_or(kid_sample *s, uint64_t byte_off, uint64_t nbytes, const void *src, int src_on_device)
{
    if (!s || (nbytes && !src)) return kid_fail(KID_ERR_ARG, "null argument");
    if ((byte_off & 15) || (nbytes & 15) || byte_off + nbytes > s->seen_words * 4)
        return kid_fail(KID_ERR_ARG, "range must be 16-byte aligned and inside the bitmap");
    int rc = kid_use_device(s->db->device);
    if (rc != KID_OK) return rc;
    if (nbytes == 0) return KID_OK;
    const uint32_t *dsrc = (const uint32_t *)src;
    KidDevBuf tmp;
    if (!src_on_device) {
        KID_HIP(tmp.alloc(nbytes));
        KID_HIP(hipMemcpy(tmp.p, src, nbytes, hipMemcpyHostToDevice));
        dsrc = tmp.as<uint32_t>();
    }
    KID_HIP(hipDeviceSynchronize());
    hipLaunchKernelGGL(kid_or_kernel, dim3(kid_grid_for(nbytes / 4, 256, s->db->num_cu * 16)), dim3(256), 0, 0,
                       s->seen.as<uint32_t>() + byte_off / 4, dsrc, nbytes / 4);
    KID_HIP(hipDeviceSynchronize());
    return KID_OK;
}

#include "kid_api_support.h"
#include "kid_api_fragments.h"
#include "kid_api_votes.h"
#include "kid_api_fragment_votes.h"
#include "kid_api_segments.h"
#include "kid_api_segment_votes.h"
#include "kid_api_loci.h"
#include "kid_api_fragment_loci.h"
#include "kid_api_pileup.h"
#include "kid_api_depth.h"
#include "kid_api_shared.h"
#include "kid_api_coverage.h"
