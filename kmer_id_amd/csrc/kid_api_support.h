// kid_api_support.h -- call reads by k-mer support: kid_db_read_support* over the hit pass and kid_support_kernel
// (kid_support.hip.h) -- and, once, the call path of every family that leaves one record per unit of the batch behind
// the hit pass (kid_calls_*): the argument checks, the host run with the binding of a tally, the launch between the
// family's two events, the *_from_hits_device form.  A family is a struct like KidSupportCalls below; the others are
// KidFragmentCalls (kid_api_fragments.h), whose unit is two reads, KidVoteCalls (kid_api_votes.h), which queues two
// kernels through the hook of kid_calls_queue, and KidFragmentVoteCalls (kid_api_fragment_votes.h), which does both.
// The host-buffer forms open their batch with kid_hits_open_* and run the hit pass with kid_hits_host_pass
// (kid_api_hits.h).  Included behind the sample handle: a tally counts into one.
#pragma once
#include "kid_api_hits.h"
#include "kid_support.hip.h"

static_assert(sizeof(kid_support) == sizeof(KidSupport), "kid_support is the device record");

struct KidSupportCalls {
    typedef KidSupport Rec;
    static constexpr uint64_t unit_reads = 1;
    static constexpr unsigned settle = KID_SETTLE_SUPPORT;
    static constexpr KidDevBuf KidHitsState::*out = &KidHitsState::out_support;     // the host forms' records
    static constexpr KidSpanTimer KidHitsState::*timer = &KidHitsState::support;    // the kernel alone
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
template <class F> static int kid_calls_check_args(const kid_db *db, uint64_t n_reads, uint32_t min_permille, const kid_sample *tally)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc == KID_OK) rc = kid_support_check_tally(db, tally);
    if (rc == KID_OK) rc = kid_check_n_reads(n_reads);
    if (rc != KID_OK) return rc;
    if (n_reads % F::unit_reads)
        return kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
    return KID_OK;
}

// What a family queues between its timer's two events.  A family without a hook: its kernel() over the grid.  The
// optional hook: a static F::queue<ROWS, TALLY, DEPTH>(db, h, grid, stream, the kernel's arguments...) -> status, in
// which the family binds scratch of its own to the batch and queues what it needs (KidVoteCalls: a second kernel
// behind the first).  The first overload is the better match and drops out where F has no such member.
template <class F, bool ROWS, bool TALLY, bool DEPTH, class... A>
static auto kid_calls_queue(int, kid_db *db, KidHitsState *h, dim3 grid, hipStream_t stream, A... a)
    -> decltype(F::template queue<ROWS, TALLY, DEPTH>(db, h, grid, stream, a...))
{
    return F::template queue<ROWS, TALLY, DEPTH>(db, h, grid, stream, a...);
}
template <class F, bool ROWS, bool TALLY, bool DEPTH, class... A>
static int kid_calls_queue(long, kid_db *, KidHitsState *, dim3 grid, hipStream_t stream, A... a)
{
    hipLaunchKernelGGL((F::template kernel<ROWS, TALLY, DEPTH>()), grid, dim3(256), 0, stream, a...);
    return KID_OK;
}

// the family's kernel over one batch of n units on `stream` between the two events; t: null, or what a tally needs
template <class F>
static int kid_calls_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers,
                            uint64_t n, KidSupportRule rule, typename F::Rec *d_out, const KidSupportTally *t, hipStream_t stream)
{
    const dim3 grid(kid_grid_for(n, 256, db->num_cu * 8));
    KidSpanTimer &timer = h->*F::timer;
    int rc = timer.begin(stream);
    if (rc != KID_OK) return rc;
    kid_lift(db->d.rows != nullptr, [&](auto rows) {
        kid_lift(t != nullptr, [&](auto tally) {
            kid_lift(t != nullptr && t->depth != nullptr, [&](auto depth) { // the depth form exists for a tally alone
                if constexpr (decltype(tally)::value || !decltype(depth)::value)
                    rc = kid_calls_queue<F, decltype(rows)::value, decltype(tally)::value, decltype(depth)::value>(
                        0, db, h, grid, stream, db->d, d_hit_offsets, d_hits, d_n_kmers, n, rule, d_out, t ? *t : KidSupportTally{});
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
    const KidDevBuf &d_out = h->*F::out;
    const uint64_t n = ob.b.n / F::unit_reads, out_nbytes = n * sizeof(typename F::Rec);
    uint64_t total = 0;
    int rc;
    if (out) KID_HIP(kid_hits_ensure(h->*F::out, out_nbytes));
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

// the family's kernel over a hit CSR in device memory (the caller's, or what kid_db_read_hits_device left)
template <class F>
static int kid_calls_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                      uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    int rc = kid_calls_check_args<F>(db, n_reads, min_permille, nullptr);
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
    int rc = kid_calls_check_args<KidSupportCalls>(db, n_reads, min_permille, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_offsets(ob, db, bases, offsets, start, stop, n_reads, KidSupportCalls::settle)) != KID_OK) return rc;
    return kid_calls_host_run<KidSupportCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_read_support_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                         uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally)
{
    int rc = kid_calls_check_args<KidSupportCalls>(db, n_reads, min_permille, tally);
    if (rc != KID_OK || n_reads == 0) return rc;
    KidOpenBatch ob;
    if ((rc = kid_hits_open_fastq(ob, db, text, text_nbytes, recs, n_reads, KidSupportCalls::settle)) != KID_OK) return rc;
    return kid_calls_host_run<KidSupportCalls>(db, ob, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_support_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                               uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    return kid_calls_from_hits_device<KidSupportCalls>(db, d_hit_offsets, d_hits, d_n_kmers, n_reads, min_hits, min_permille, d_out, stream);
}

extern "C" int kid_db_read_support_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads)
{
    return kid_hits_take_time(db, &KidHitsState::support, false, device_ms, calls, reads);
}
