// kid_api_fragments.h -- call mate pairs as one fragment: kid_db_read_fragments* over the hit pass and kid_fragment_kernel
// (kid_fragments.hip.h).  The batch is 2 F reads in interleaved order (read 2i = mate 1 of fragment i, read 2i + 1 = its
// mate 2); the checks, staging, hit pass, rule and tally checks are those of kid_api_hits.h / kid_api_support.h, and the
// calls obey their one-call-at-a-time rule.  The FASTQ form stages its two text blocks as one (block 2 behind block 1)
// with an interleaved record index of shifted offsets: one hit pass.  The fragment kernel has the KidSpanTimer
// `fragments` of the database's KidHitsState.  Included behind kid_api_support.h.
#pragma once
#include "kid_api_support.h"
#include "kid_fragments.hip.h"

static_assert(sizeof(kid_fragment) == sizeof(KidFragment), "kid_fragment is the device record");

// the hits scratch, free: hit pass, support kernel and fragment kernel of the call before are through
static int kid_fragments_state(kid_db *db, KidHitsState **out)
{
    int rc = kid_support_state(db, out);
    if (rc != KID_OK) return rc;
    return (*out)->fragments.settle();
}

// the fragment kernel of one batch of n_fragments fragments on `stream` between the two events; t: null, or what a tally needs
static int kid_fragments_launch(kid_db *db, KidHitsState *h, const uint64_t *d_hit_offsets, const KidHit *d_hits, const uint32_t *d_n_kmers,
                                uint64_t n_fragments, KidSupportRule rule, KidFragment *d_out, const KidSupportTally *t, hipStream_t stream)
{
    const dim3 grid(kid_grid_for(n_fragments, 256, db->num_cu * 8)), block(256);
    const KidSupportTally none{nullptr, nullptr, nullptr, nullptr};
    int rc = h->fragments.begin(stream);
    if (rc != KID_OK) return rc;
    kid_lift(db->d.rows != nullptr, [&](auto rows) {
        kid_lift(t != nullptr, [&](auto tally) {
            kid_lift(t != nullptr && t->depth != nullptr, [&](auto depth) { // the depth form exists for a tally alone
                if constexpr (decltype(tally)::value || !decltype(depth)::value)
                    hipLaunchKernelGGL((kid_fragment_kernel<decltype(rows)::value, decltype(tally)::value, decltype(depth)::value>), grid, block, 0,
                                       stream, db->d, d_hit_offsets, d_hits, d_n_kmers, n_fragments, rule, d_out, t ? *t : none);
            });
        });
    });
    KID_HIP(hipGetLastError());
    return h->fragments.end(stream, n_fragments);
}

// The host-buffer forms behind their uploads (b: the 2 F staged reads): the hit pass into the library's scratch, the
// fragment kernel, 32 bytes per fragment back.  A tally's kernel goes into the sample's stream, as kid_support_host_run's.
static int kid_fragments_host_run(kid_db *db, KidHitsState *h, const KidBatch &b, const KidFastqRec *recs, uint64_t max_tiles,
                                  KidSupportRule rule, kid_fragment *out, kid_sample *tally)
{
    const uint64_t nf = b.n / 2;
    uint64_t total = 0;
    int rc;
    if (out) KID_HIP(kid_hits_ensure(h->out_fragments, nf * sizeof(KidFragment)));
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
    rc = kid_fragments_launch(db, h, h->out_offsets.as<uint64_t>(), total ? h->out_hits.as<KidHit>() : nullptr, h->out_nk.as<uint32_t>(), nf, rule,
                              out ? h->out_fragments.as<KidFragment>() : nullptr, tally ? &t : nullptr, st);
    if (rc != KID_OK) return rc;
    KID_HIP(hipStreamSynchronize(st));
    if (out) KID_HIP(hipMemcpy(out, h->out_fragments.p, nf * sizeof(KidFragment), hipMemcpyDeviceToHost));
    return KID_OK;
}

static int kid_fragments_check_args(const kid_db *db, uint64_t n_reads, uint32_t min_permille, const void *out, const kid_sample *tally)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc != KID_OK) return rc;
    if ((rc = kid_support_check_tally(db, tally)) != KID_OK) return rc;
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (n_reads & 1ull) return kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
    if (n_reads && !out && !tally) return kid_fail(KID_ERR_ARG, "null argument");
    return KID_OK;
}

extern "C" int kid_db_read_fragments(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                                     uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment *out, kid_sample *tally)
{
    int rc = kid_fragments_check_args(db, n_reads, min_permille, out, tally);
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    uint64_t max_tiles = 0;
    if ((rc = kid_hits_check_offsets(db, bases, offsets, start, stop, n_reads, &max_tiles)) != KID_OK) return rc;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    KidBatch b{};
    if ((rc = kid_fragments_state(db, &h)) != KID_OK) return rc;
    if ((rc = kid_hits_stage_offsets(h, bases, offsets, start, stop, n_reads, &b)) != KID_OK) return rc;
    return kid_fragments_host_run(db, h, b, nullptr, max_tiles, KidSupportRule{min_hits, min_permille}, out, tally);
}

// One mate's block: its records inside its text; with `masking` its lines in ascending order without overlap (per block:
// the merged index interleaves the two).  An absent mate (seq_len = qual_len = 0) has no line.  Adds to *max_tiles.
static int kid_fragments_check_block(const kid_fastq_rec *recs, uint64_t n, uint64_t nbytes, int mate, bool masking, uint64_t *max_tiles,
                                     uint32_t *longest)
{
    uint64_t free_from = 0;
    for (uint64_t r = 0; r < n; r++) {
        const kid_fastq_rec &c = recs[r];
        if ((uint64_t)c.seq_off + c.seq_len > nbytes || (uint64_t)c.qual_off + c.qual_len > nbytes)
            return kid_fail(KID_ERR_ARG, "mate %d, record %llu lies outside the text block", mate, (unsigned long long)r);
        *max_tiles += c.seq_len / KID_HITS_TILE + 1;
        if (masking && (c.seq_len || c.qual_len)) {
            if (c.seq_off < free_from || (uint64_t)c.seq_off + c.seq_len > c.qual_off)
                return kid_fail(KID_ERR_ARG, "mate %d, record %llu: with min_base_quality on, the lines of a block must be in ascending order "
                                             "and must not overlap", mate, (unsigned long long)r);
            free_from = (uint64_t)c.qual_off + c.qual_len;
        }
        if (c.seq_len > *longest) *longest = c.seq_len;
    }
    return KID_OK;
}

extern "C" int kid_db_read_fragments_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                           uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t min_hits,
                                           uint32_t min_permille, kid_fragment *out, kid_sample *tally)
{
    if (n_fragments > 0x3FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^30-1 fragments per batch");
    int rc = kid_fragments_check_args(db, 2 * n_fragments, min_permille, out, tally);
    if (rc != KID_OK) return rc;
    if (n_fragments == 0) return KID_OK;
    if (!recs1 || !recs2 || (!text1 && nbytes1) || (!text2 && nbytes2)) return kid_fail(KID_ERR_ARG, "null argument");
    // one staged text: the shifted offsets of block 2 are 32-bit like every kid_fastq_rec
    if (nbytes1 + nbytes2 < nbytes1 || nbytes1 + nbytes2 >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "two FASTQ blocks of 4 GiB or more together");
    uint64_t max_tiles = 0;
    uint32_t longest = 0;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    const bool masking = db->min_base_quality > 0;
    if ((rc = kid_fragments_check_block(recs1, n_fragments, nbytes1, 1, masking, &max_tiles, &longest)) != KID_OK) return rc;
    if ((rc = kid_fragments_check_block(recs2, n_fragments, nbytes2, 2, masking, &max_tiles, &longest)) != KID_OK) return rc;
    if ((rc = kid_use_device(db->device)) != KID_OK) return rc;
    KidHitsState *h = nullptr;
    if ((rc = kid_fragments_state(db, &h)) != KID_OK) return rc;
    const uint64_t n = 2 * n_fragments, nbytes = nbytes1 + nbytes2;
    const uint32_t shift = (uint32_t)nbytes1;
    std::vector<kid_fastq_rec> merged(n); // (synchronous copies read it)
    for (uint64_t i = 0; i < n_fragments; i++) {
        merged[2 * i] = recs1[i];
        kid_fastq_rec c = recs2[i];
        c.seq_off += shift;
        c.qual_off += shift;
        merged[2 * i + 1] = c;
    }
    KID_HIP(kid_hits_ensure(h->in_bases, kid_text_bytes(nbytes)));
    {   // kid_upload_text for two sources: zero from the last whole 16-byte group on, then the blocks back to back
        const uint64_t tail = nbytes & ~15ull;
        KID_HIP(hipMemsetAsync(h->in_bases.as<uint8_t>() + tail, 0, kid_text_bytes(nbytes) - tail, 0));
        if (nbytes1) KID_HIP(hipMemcpyAsync(h->in_bases.p, text1, nbytes1, hipMemcpyHostToDevice, 0));
        if (nbytes2) KID_HIP(hipMemcpyAsync(h->in_bases.as<uint8_t>() + nbytes1, text2, nbytes2, hipMemcpyHostToDevice, 0));
    }
    KID_HIP(kid_hits_ensure(h->in_recs, n * sizeof(KidFastqRec)));
    KID_HIP(kid_hits_ensure(h->trim_start, n * 4));
    KID_HIP(kid_hits_ensure(h->trim_stop, n * 4));
    KID_HIP(hipMemcpy(h->in_recs.p, merged.data(), n * sizeof(KidFastqRec), hipMemcpyHostToDevice));
    KidBatch b{};
    b.bases = h->in_bases.as<uint8_t>();
    b.start = h->trim_start.as<int32_t>(); // (outputs of the prepare kernel here)
    b.stop = h->trim_stop.as<int32_t>();
    b.n = n;
    const KidFastqRec *d_recs = h->in_recs.as<KidFastqRec>();
    if (masking && (rc = kid_mask_launch_fastq(db, h->in_bases.as<uint8_t>(), d_recs, n, longest, db->min_base_quality, nullptr, 0)) != KID_OK)
        return rc;
    return kid_fragments_host_run(db, h, b, d_recs, max_tiles, KidSupportRule{min_hits, min_permille}, out, tally);
}

extern "C" int kid_db_fragments_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers,
                                                 uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_support_check_rule(min_permille);
    if (rc != KID_OK) return rc;
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    if (n_reads & 1ull) return kid_fail(KID_ERR_ARG, "n_reads = %llu is odd: a batch of fragments holds two reads each", (unsigned long long)n_reads);
    if (n_reads && (!d_hit_offsets || !d_n_kmers || !d_out)) return kid_fail(KID_ERR_ARG, "null argument");
    rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    if (n_reads == 0) return KID_OK;
    std::lock_guard<std::mutex> lock(db->hits_mu);
    KidHitsState *h = nullptr;
    if ((rc = kid_fragments_state(db, &h)) != KID_OK) return rc;
    return kid_fragments_launch(db, h, (const uint64_t *)d_hit_offsets, (const KidHit *)d_hits, (const uint32_t *)d_n_kmers, n_reads / 2,
                                KidSupportRule{min_hits, min_permille}, (KidFragment *)d_out, nullptr, (hipStream_t)stream);
}

extern "C" int kid_db_read_fragments_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments)
{
    return kid_hits_take_time(db, &KidHitsState::fragments, false, device_ms, calls, fragments);
}
