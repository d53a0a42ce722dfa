// kid_api_support.h -- call reads by k-mer support: kid_db_read_support* over the hit pass and kid_support_kernel
// (kid_support.hip.h) -- and, once, the call path of every family that leaves one record per unit of the batch behind
// the hit pass (kid_calls_*): the argument checks, the host run with the binding of a tally, the launch between the
// family's two events, and the four forms (kid_calls_offsets, _fastq, _fastq_pairs, _from_hits_device) that the
// families' extern "C" functions forward to.  A family is a struct like KidSupportCalls below; the others are
// KidFragmentCalls (kid_api_fragments.h), whose unit is two reads, KidVoteCalls (kid_api_votes.h), which has a second
// kernel over a KidVoteScratch, and KidFragmentVoteCalls (kid_api_fragment_votes.h), which has both.
// The host-buffer forms open their batch with kid_hits_open_* and run the hit pass with kid_hits_host_pass
// (kid_api_hits.h).  Included behind the sample handle: a tally counts into one.
#pragma once
#include "kid_api_hits.h"
#include "kid_support.hip.h"
#include "kid_votes.hip.h"

static_assert(sizeof(kid_support) == sizeof(KidSupport), "kid_support is the device record");

// A family of these calls is a struct with
//   Rec            its device record (= the C ABI's)
//   id             its KidFamilyState in KidHitsState: the host forms' records, the timer of its kernels
//   unit_reads     the reads of the batch that one record is about
//   needs_sink     whether a call with neither `out` nor `tally` is refused
//   settle         the timers it waits for before the scratch is its own (kid_hits_state)
//   kernel()       its kernel over the units of a batch, and where it has a second one for the units with many hits:
//   big            the KidVoteScratch of KidHitsState the two share (the others: null), big_kernel() the second
struct KidSupportCalls {
    typedef KidSupport Rec;
    static constexpr KidFamily id = KID_FAM_SUPPORT;
    static constexpr uint64_t unit_reads = 1;
    static constexpr bool needs_sink = false;
    static constexpr unsigned settle = kid_settle(KID_FAM_SUPPORT);
    static constexpr KidVoteScratch KidHitsState::*big = nullptr;
    template <bool ROWS, bool TALLY, bool DEPTH> static constexpr auto kernel() { return &kid_support_kernel<ROWS, TALLY, DEPTH>; }
};

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

// what every form of a family refuses first, in the order callers see
template <class F>
static int kid_calls_check_args(const kid_db *db, uint64_t n_reads, uint32_t min_permille, const void *out, const kid_sample *tally)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc == KID_OK) rc = kid_support_check_tally(db, tally);
    if (rc == KID_OK) rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (n_reads % F::unit_reads)
        return kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
    if (F::needs_sink && n_reads && !out && !tally) return kid_fail(KID_ERR_ARG, "null argument");
    return KID_OK;
}

// What a family queues between its timer's two events: its kernel over the grid, and where it has a second kernel, the
// scratch bound to the batch of n units, both kernels with the scratch as their last argument, the second over one
// workgroup per row: it reads the list's length on the device, there is no host round trip.
template <class F, bool ROWS, bool TALLY, bool DEPTH, class... A>
static int kid_calls_queue(kid_db *db, KidHitsState *h, dim3 grid, hipStream_t stream, uint64_t n, A... a)
{
    if constexpr (F::big != nullptr) {
        KidVoteScratch &s = h->*F::big;
        const int rc = kid_vote_scratch_bind(db, s, n * 4u, stream);
        if (rc != KID_OK) return rc;
        const KidVoteBig big{s.list.as<uint32_t>(), s.n_list.as<uint32_t>(), s.rows->as<uint32_t>()};
        hipLaunchKernelGGL((F::template kernel<ROWS, TALLY, DEPTH>()), grid, dim3(256), 0, stream, a..., big);
        hipLaunchKernelGGL((F::template big_kernel<ROWS, TALLY, DEPTH>()), dim3(db->num_cu), dim3(256), 0, stream, a..., big);
    } else
        hipLaunchKernelGGL((F::template kernel<ROWS, TALLY, DEPTH>()), grid, dim3(256), 0, stream, a...);
    return KID_OK;
}

// the family's kernel over one batch of n units on `stream` between the two events; t: null, or what a tally needs
template <class F>
static int kid_calls_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers,
                            uint64_t n, KidSupportRule rule, typename F::Rec *d_out, const KidSupportTally *t, hipStream_t stream)
{
    const dim3 grid(kid_grid_for(n, 256, db->num_cu * 8));
    KidSpanTimer &timer = h->family[F::id].timer;
    int rc = timer.begin(stream);
    if (rc != KID_OK) return rc;
    kid_lift(db->d.rows != nullptr, [&](auto rows) {
        kid_lift(t != nullptr, [&](auto tally) {
            kid_lift(t != nullptr && t->depth != nullptr, [&](auto depth) { // the depth form exists for a tally alone
                if constexpr (decltype(tally)::value || !decltype(depth)::value)
                    rc = kid_calls_queue<F, decltype(rows)::value, decltype(tally)::value, decltype(depth)::value>(
                        db, h, grid, stream, n, db->d, d_hit_offsets, d_hits, d_n_kmers, n, rule, d_out, t ? *t : KidSupportTally{});
            });
        });
    });
    if (rc != KID_OK) return rc;
    KID_HIP(hipGetLastError());
    return timer.end(stream, n);
}

// The host-buffer forms behind their uploads: the hit pass into the library's scratch (kid_hits_host_pass, every hit
// filled in), the family's kernel, one record per unit back.  A tally's kernel goes into the sample's stream behind
// whatever the sample has queued (classify kernels, a hit-log pass: both write the counters it adds to).
template <class F>
static int kid_calls_host_run(kid_db *db, const KidOpenBatch &ob, KidSupportRule rule, void *out, kid_sample *tally)
{
    KidHitsState *h = ob.h;
    KidDevBuf &d_out = h->family[F::id].out;
    const uint64_t n = ob.b.n / F::unit_reads, out_nbytes = n * sizeof(typename F::Rec);
    uint64_t total = 0;
    int rc;
    if (out) KID_HIP(kid_hits_ensure(d_out, out_nbytes));
    if ((rc = kid_hits_host_pass(db, ob, KID_HITS_NO_LIMIT, &total)) != KID_OK) return rc;
    // what the prepare kernels refuse (a range outside its read, a short quality line) is refused before anything is counted
    if ((rc = kid_hits_check(h)) != KID_OK) return rc;
    hipStream_t st = 0;
    KidSupportTally t{};
    if (tally) {
        st = tally->stream.s;
        if ((rc = kid_sample_order_behind(tally, st)) != KID_OK) return rc;
        t.gcount = tally->gcount.as<unsigned long long>();
        t.seen = tally->seen.as<uint32_t>();
        t.fastq_desc = ob.d_recs ? h->desc.as<KidReadDesc>() : nullptr;
        t.depth = tally->depth.as<uint32_t>(); // null unless KID_OPT_ENTRY_DEPTH is on
    }
    rc = kid_calls_launch<F>(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), n, rule,
                             out ? d_out.as<typename F::Rec>() : nullptr, tally ? &t : nullptr, st);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(st));
    if (out) KID_HIP(hipMemcpy(out, d_out.p, out_nbytes, hipMemcpyDeviceToHost));
    return KID_OK;
}

// The forms of a family, once; every one checks with kid_calls_check_args first.  A batch of reads in host memory:
template <class F>
static int kid_calls_offsets(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                             uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, void *out, kid_sample *tally)
{
    int rc = kid_calls_check_args<F>(db, n_reads, min_permille, out, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, F::settle)) != KID_OK) return rc;
    return kid_calls_host_run<F>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

// a block of FASTQ text with its line index
template <class F>
static int kid_calls_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                           uint32_t min_hits, uint32_t min_permille, void *out, kid_sample *tally)
{
    int rc = kid_calls_check_args<F>(db, n_reads, min_permille, out, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, F::settle)) != KID_OK) return rc;
    return kid_calls_host_run<F>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

// two blocks of FASTQ text, the mates of n_fragments fragments (a family whose unit is two reads)
template <class F>
static int kid_calls_fastq_pairs(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                 uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t min_hits, uint32_t min_permille,
                                 void *out, kid_sample *tally)
{
    static_assert(F::unit_reads == 2, "a pair of blocks holds fragments");
    if (n_fragments > 0x3FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^30-1 fragments per batch");
    int rc = kid_calls_check_args<F>(db, 2 * n_fragments, min_permille, out, tally);
    if (rc != KID_OK || n_fragments == 0) return rc;
    if (!recs1 || !recs2 || (!text1 && nbytes1) || (!text2 && nbytes2)) return kid_fail(KID_ERR_ARG, "null argument");
    // one staged text: the shifted offsets of block 2 are 32-bit like every kid_fastq_rec
    if (nbytes1 + nbytes2 < nbytes1 || nbytes1 + nbytes2 >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "two FASTQ blocks of 4 GiB or more together");
    KidOpenBatch ob;
    rc = kid_hits_open_fastq(ob, db, text1, nbytes1, recs1, 2 * n_fragments, F::settle, nullptr, text2, nbytes2, recs2);
    if (rc != KID_OK) return rc;
    return kid_calls_host_run<F>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

// the family's kernel over a hit CSR in device memory (the caller's, or what kid_db_read_hits_device left)
template <class F>
static int kid_calls_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                      uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    int rc = kid_calls_check_args<F>(db, n_reads, min_permille, d_out, nullptr);
    if (rc != KID_OK) return rc;
    if (n_reads && (!d_hit_offsets || !d_n_kmers || !d_out)) return kid_fail(KID_ERR_ARG, "null argument");
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_hits_state(db, F::settle, &h)) != KID_OK) return rc;
    return kid_calls_launch<F>(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers,
                               n_reads / F::unit_reads, KidSupportRule{min_hits, min_permille}, (typename F::Rec *)d_out, nullptr,
                               (hipStream_t)stream);
}

extern "C" int kid_db_read_support(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                   uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally)
{
    return kid_calls_offsets<KidSupportCalls>(db, bases, offsets, start, stop, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_read_support_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                         uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally)
{
    return kid_calls_fastq<KidSupportCalls>(db, text, text_nbytes, recs, n_reads, min_hits, min_permille, out, tally);
}

extern "C" int kid_db_support_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                               uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidSupportCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_support_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, KidSupportCalls::id, device_ms, calls, reads);
}
