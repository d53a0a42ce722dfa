#include "kid_driver.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <iostream>
#include <mutex>
#include <thread>

namespace kidhost {

void leave_now(int exit_code)
{
    std::cout.flush();
    std::cerr.flush();
    fflush(nullptr);
    _exit(exit_code);
}

void die_kid(int rc)
{
    std::cerr << "kmer_id_amd: " << kid_strerror(rc) << ": " << kid_last_error() << "\n";
    // (a quality line shorter than its sequence, found by the GPU's process_qual: the reference dies in std::string::at,
    //  abort -> 134; "out of memory in table" is exit 1, newkmer_10nx.cpp:256-260).  Other threads may still be reading
    //  files or using the GPU: nothing is unwound, no destructor runs under them.
    leave_now(rc == KID_ERR_TABLE_FULL ? 1 : rc == KID_ERR_FORMAT ? 134 : 3);
}

static double seconds_since(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void load_database(const std::string &tree_path, const std::string &probes_path, const std::string &cache_path, int k, int ntar,
                   std::vector<int32_t> &parent, ProbeSet &ps, bool *from_cache, int threads, StartupTiming *timing,
                   std::thread *cache_writer, bool want_sites)
{
    if (from_cache) *from_cache = false;
    const auto t0 = std::chrono::steady_clock::now();
    if (!cache_path.empty() && load_db_cache(cache_path, tree_path, probes_path, k, ntar, parent, ps)) {
        if (from_cache) *from_cache = true;
        if (timing) timing->cache_read_s = seconds_since(t0);
        if (want_sites) { // the cache holds no sites: the text is read for them alone
            ProbeSet text = load_probes_gz(probes_path, k, threads, timing, true);
            if (text.orgs.size() != ps.keys.size()) throw Fatal{3, probes_path + " has another number of entries than the database cache " + cache_path};
            ps.orgs = std::move(text.orgs);
            ps.positions = std::move(text.positions);
        }
        return;
    }
    parent = load_tree(tree_path, ntar);
    ps = load_probes_gz(probes_path, k, threads, timing, want_sites);
    if (cache_path.empty()) return;
    // the cache is written beside the upload and the table build when the caller can wait for it later (it must: `ps`
    // and `parent` are read until the writer is joined)
    auto write = [cache_path, tree_path, probes_path, k, &parent, &ps, timing]() {
        const auto t1 = std::chrono::steady_clock::now();
        if (!save_db_cache(cache_path, tree_path, probes_path, k, parent, ps))
            std::cerr << "kmer_id_amd: could not write the database cache " << cache_path << "\n";
        if (timing) timing->cache_write_s = seconds_since(t1);
    };
    if (cache_writer) *cache_writer = std::thread(write);
    else write();
}

Engine::~Engine()
{
    for (kid_sample *s : samples) kid_sample_destroy(s);
    for (const std::vector<kid_sample *> &list : tallied)
        for (kid_sample *s : list) kid_sample_destroy(s);
    for (kid_pileup *p : pileups) kid_pileup_destroy(p); // (before their databases)
    if (owns_dbs)
        for (kid_db *d : dbs) kid_db_destroy(d);
}

static void ok_or_die(int rc) { if (rc != KID_OK) die_kid(rc); }
static kid_sample *begin_sample_or_die(kid_db *db)
{
    kid_sample *s = nullptr;
    ok_or_die(kid_sample_begin(db, &s));
    return s;
}

std::unique_ptr<Engine> engine_worker(const Engine &owner)
{
    std::unique_ptr<Engine> e(new Engine());
    e->owns_dbs = false;
    e->dbs = owner.dbs;
    e->db = owner.db;
    e->ntar = owner.ntar;
    e->k = owner.k;
    e->batch_reads = owner.batch_reads;
    e->batch_bases = owner.batch_bases;
    e->site_pos = owner.site_pos;
    for (kid_db *d : e->dbs) e->samples.push_back(begin_sample_or_die(d));
    e->sample = e->samples[0];
    engine_configure(*e, owner.side);
    return e;
}

void engine_configure(Engine &e, const SideOptions &side)
{
    e.side = side;
    for (int t = 0; t < TALLY_COUNT; t++)
        if (kTallies[t].wanted(side))
            for (kid_db *d : e.dbs) e.tallied[t].push_back(begin_sample_or_die(d));
    if (side.depth)
        for (kid_sample *s : e.tallied[TALLY_CONFIDENT]) ok_or_die(kid_sample_set_option(s, KID_OPT_ENTRY_DEPTH, 1));
    if (side.pileup.on && e.site_pos) // (the databases have their sites: engine_open)
        for (kid_db *d : e.dbs) {
            kid_pileup *p = nullptr;
            ok_or_die(kid_pileup_create(d, side.pileup.bin_width, &p));
            e.pileups.push_back(p);
        }
    // the two masks: the sample's option and the database's, each only where it is on
    const struct { int value, sample_opt, db_opt; } masks[] = {{side.min_base_quality, KID_OPT_MIN_BASE_QUALITY, KID_DB_OPT_MIN_BASE_QUALITY},
                                                               {side.low_complexity, KID_OPT_LOW_COMPLEXITY, KID_DB_OPT_LOW_COMPLEXITY}};
    for (const auto &m : masks) {
        if (m.value == 0) continue;
        for (kid_sample *s : e.samples) ok_or_die(kid_sample_set_option(s, m.sample_opt, m.value));
        for (int t = 0; t < TALLY_COUNT; t++)
            if (kTallies[t].own_masks)
                for (kid_sample *s : e.tallied[t]) ok_or_die(kid_sample_set_option(s, m.sample_opt, m.value));
        if (!e.owns_dbs) continue; // (a worker: its owner has set it)
        for (kid_db *d : e.dbs) ok_or_die(kid_db_set_option(d, m.db_opt, m.value));
    }
}

std::vector<int> parse_devices(int device, const std::string &list)
{
    if (list.empty()) return std::vector<int>(1, device);
    std::vector<int> out;
    size_t pos = 0;
    while (pos <= list.size()) {
        size_t comma = list.find(',', pos);
        if (comma == std::string::npos) comma = list.size();
        if (comma > pos) out.push_back(atoi(list.substr(pos, comma - pos).c_str()));
        pos = comma + 1;
    }
    return out;
}

void engine_reset(Engine &e)
{
    for (kid_sample *s : e.samples) ok_or_die(kid_sample_reset(s));
    for (const std::vector<kid_sample *> &list : e.tallied)
        for (kid_sample *s : list) ok_or_die(kid_sample_reset(s));
    for (kid_pileup *p : e.pileups) ok_or_die(kid_pileup_reset(p));
    e.next_sample = 0;
    e.next_fragments = 0;
}

bool engine_open(Engine &e, const ProbeSet &ps, const std::vector<int32_t> &parent, int k, int log2_slots, int max_probes,
                 unsigned flags, const std::vector<int> &devices)
{
    if (devices.empty()) { std::cerr << "kmer_id_amd: no device given\n"; leave_now(2); }
    e.ntar = (int)parent.size();
    e.k = k;
    int rc = kid_db_build(ps.keys.data(), ps.targets.data(), ps.keys.size(), parent.data(), e.ntar, k, log2_slots, max_probes,
                          flags, devices[0], &e.db);
    if (rc == KID_ERR_TABLE_FULL) {
        std::cout << "out of memory in table " << std::endl;
        return false;
    }
    if (rc != KID_OK) die_kid(rc);
    e.sample = begin_sample_or_die(e.db);
    e.dbs.assign(1, e.db);
    e.samples.assign(1, e.sample);
    for (size_t i = 1; i < devices.size(); i++) { // the reference, pinned into every GPU's HBM: device-to-device copies of the one built table
        kid_db *r = nullptr;
        rc = kid_db_replicate(e.db, devices[i], &r);
        if (rc != KID_OK) die_kid(rc);
        e.dbs.push_back(r);
        e.samples.push_back(begin_sample_or_die(r));
    }
    if (ps.orgs.size() == ps.keys.size() && ps.positions.size() == ps.keys.size() && ps.keys.size() > 0) { // loaded with sites: --loci
        for (kid_db *d : e.dbs)
            if ((rc = kid_db_set_sites(d, ps.orgs.data(), ps.positions.data(), ps.keys.size())) != KID_OK) die_kid(rc);
        e.site_pos = std::make_shared<const std::vector<uint32_t>>(ps.positions.data(), ps.positions.data() + ps.positions.size());
    }
    return true;
}

struct Prefetcher::Impl {
    struct Slot {
        std::deque<std::unique_ptr<ReadBatch>> q;
        bool done = false, failed = false;
        Fatal failure{0, ""};
        SourceStats stats;
    };
    double waited_s = 0;
    std::vector<SourceOpener> files;
    std::vector<Slot> slots;
    std::vector<std::thread> pool;
    std::mutex m;
    std::condition_variable cv;
    size_t next_file = 0, batch_reads, batch_bases, depth;
    bool stop = false;

    void reader()
    {
        for (;;) {
            size_t i;
            {
                std::lock_guard<std::mutex> lk(m);
                if (stop || next_file >= files.size()) return;
                i = next_file++;
            }
            try {
                std::unique_ptr<ReadSource> src = files[i]();
                if (src) {
                    for (;;) {
                        std::unique_ptr<ReadBatch> b(new ReadBatch());
                        if (!src->fill(*b, batch_reads, batch_bases)) break;
                        std::unique_lock<std::mutex> lk(m);
                        cv.wait(lk, [&] { return stop || slots[i].q.size() < depth; });
                        if (stop) return;
                        slots[i].q.push_back(std::move(b));
                        cv.notify_all();
                    }
                    src->close();
                    const SourceStats st = src->stats();
                    std::lock_guard<std::mutex> lk(m);
                    slots[i].stats = st;
                }
            } catch (const Fatal &f) {
                std::lock_guard<std::mutex> lk(m);
                slots[i].failed = true;
                slots[i].failure = f;
            }
            std::lock_guard<std::mutex> lk(m);
            slots[i].done = true;
            cv.notify_all();
        }
    }
};

Prefetcher::Prefetcher(std::vector<SourceOpener> files, int threads, size_t batch_reads, size_t batch_bases, size_t depth)
    : impl_(new Impl())
{
    impl_->files = std::move(files);
    impl_->slots = std::vector<Impl::Slot>(impl_->files.size());
    impl_->batch_reads = batch_reads;
    impl_->batch_bases = batch_bases;
    impl_->depth = depth < 1 ? 1 : depth;
    if (threads < 1) threads = 1;
    if ((size_t)threads > impl_->files.size()) threads = (int)impl_->files.size();
    for (int t = 0; t < threads; t++) impl_->pool.emplace_back([this] { impl_->reader(); });
}

Prefetcher::~Prefetcher()
{
    {
        std::lock_guard<std::mutex> lk(impl_->m);
        impl_->stop = true;
        impl_->cv.notify_all();
    }
    for (std::thread &t : impl_->pool) t.join();
}

SourceStats Prefetcher::file_stats(size_t index)
{
    std::lock_guard<std::mutex> lk(impl_->m);
    return impl_->slots[index].stats;
}

double Prefetcher::seconds_waited() const { return impl_->waited_s; }

std::unique_ptr<ReadBatch> Prefetcher::next_any(size_t lo, size_t hi, size_t &which)
{
    std::unique_lock<std::mutex> lk(impl_->m);
    for (;;) {
        bool all_done = true;
        for (size_t i = lo; i < hi; i++) {
            Impl::Slot &s = impl_->slots[i];
            if (!s.q.empty()) {
                std::unique_ptr<ReadBatch> b = std::move(s.q.front());
                s.q.pop_front();
                impl_->cv.notify_all();
                which = i;
                return b;
            }
            if (!s.done) all_done = false;
        }
        // a failure surfaces when everything in front of it has been read to its end and handed out
        for (size_t i = lo; i < hi; i++) {
            Impl::Slot &s = impl_->slots[i];
            if (!s.done) break;
            if (s.failed) { which = i; throw s.failure; }
        }
        if (all_done) return nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        impl_->cv.wait(lk);
        impl_->waited_s += seconds_since(t0);
    }
}

// A FASTQ block's record index and its results travel through ONE buffer of text memory (page-locked once a front-end
// has installed the library's allocator): [records | final target | start | stop].  Copies to and from pageable memory
// would make every "asynchronous" call wait for the GPU.
static int submit_fastq_block(kid_sample *sample, ReadBatch &b, HostBuf &io, uint64_t *ticket)
{
    FastqBlock &fb = *b.fq;
    const size_t nr = b.size();
    io.resize(nr * (sizeof(kid_fastq_rec) + 12) + 64);
    kid_fastq_rec *recs = (kid_fastq_rec *)io.data();
    memcpy(recs, fb.recs.data(), nr * sizeof(kid_fastq_rec));
    uint32_t *fin = (uint32_t *)(recs + nr);
    int32_t *start = (int32_t *)(fin + nr), *stop = start + nr;
    return kid_classify_fastq_async(sample, (const uint8_t *)fb.text.data(), fb.used, recs, nr, fin, start, stop, ticket);
}
static void collect_fastq_block(ReadBatch &b, const HostBuf &io, std::vector<uint32_t> &final_targ)
{
    const size_t nr = b.size();
    const uint32_t *fin = (const uint32_t *)((const kid_fastq_rec *)io.data() + nr);
    const int32_t *start = (const int32_t *)(fin + nr), *stop = start + nr;
    final_targ.assign(fin, fin + nr);
    b.start.assign(start, start + nr);
    b.stop.assign(stop, stop + nr);
}

// One call of the kid_db_read_* family on a classified batch (its start / stop / final targets are known) on the batch's
// device: the FASTQ-block form for a block, else the offsets form; `rest` are the arguments behind the number of reads.
// (bases: the text of a batch of reads that was classified -- the batch's own, or its masked copy under --min-base-quality / --low-complexity)
template <class BlockForm, class OffsetsForm, class... Rest>
static void read_pass(BlockForm block_form, OffsetsForm offsets_form, kid_db *db, const ReadBatch &b, const uint8_t *bases, Rest... rest)
{
    const size_t nr = b.size();
    int rc = b.fq ? block_form(db, (const uint8_t *)b.fq->text.data(), b.fq->used, b.fq->recs.data(), nr, rest...)
                  : offsets_form(db, bases, b.offsets.data(), b.start.data(), b.stop.data(), nr, rest...);
    if (rc != KID_OK) die_kid(rc);
}
// ... of one whose last arguments are (items, cap, &total): the sizing call, then the call that fills a buffer of that size
template <class Item, class BlockForm, class OffsetsForm, class... Middle>
static std::vector<Item> read_items(BlockForm block_form, OffsetsForm offsets_form, kid_db *db, const ReadBatch &b, const uint8_t *bases,
                                    Middle... middle)
{
    std::vector<Item> items;
    uint64_t total = 0;
    read_pass(block_form, offsets_form, db, b, bases, middle..., (Item *)nullptr, (uint64_t)0, &total);
    items.resize(total);
    if (total) read_pass(block_form, offsets_form, db, b, bases, middle..., items.data(), total, &total);
    return items;
}
// A batch that has been classified, as the passes behind its classification see it: on its device, with the text that was
// classified, its final targets, the engine's options and the records of its loci pass once that has run
struct Classified {
    kid_db *db;
    const ReadBatch &b;
    const uint8_t *bases;
    const std::vector<uint32_t> &final_targ;
    const Engine &e;
    std::vector<kid_locus> &loci;
    // a record of a FASTQ block that process_qual drops: it was never handed to process_read and has no hit
    bool dropped(size_t r) const { return b.fq && !(b.stop[r] - b.start[r] >= e.k); }
    const SupportRule &rule() const { return e.side.support; } // of --min-hits / --confidence, else (0, 0)
};

// The head of a read's line: <final_targ> <trimmed length> <a> <b>, each with its tab
static void append_head(std::string &out, const Classified &c, size_t r, unsigned long long a, unsigned long long b)
{
    char num[96];
    const int n = snprintf(num, sizeof(num), "%u\t%d\t%llu\t%llu\t", c.final_targ[r], c.b.stop[r] - c.b.start[r] + 1, a, b);
    out.append(num, (size_t)n);
}
// The end of a read's line: its header line as in _reads.txt
static void append_header(std::string &out, const ReadBatch &b, size_t r)
{
    out += '\t';
    if (b.fq) out.append(b.fq->text.data() + b.fq->acc_off[r], b.fq->acc_len[r]);
    else out += b.acc[r];
    out += '\n';
}

// The hit lines of one classified batch: kid_db_read_hits*
static void hit_lines_of(const Classified &c, std::string &out)
{
    const size_t nr = c.b.size();
    std::vector<uint64_t> off(nr + 1);
    std::vector<uint32_t> nk(nr);
    const std::vector<kid_hit> hits = read_items<kid_hit>(kid_db_read_hits_fastq, kid_db_read_hits, c.db, c.b, c.bases, off.data(), nk.data());
    if (hits.empty()) return;
    char num[64];
    for (size_t r = 0; r < nr; r++) {
        if (off[r + 1] == off[r] || c.dropped(r)) continue;
        append_head(out, c, r, nk[r], off[r + 1] - off[r]);
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            const int n = snprintf(num, sizeof(num), "%s%u:%u:%u", i > off[r] ? " " : "", hits[i].pos, hits[i].target, hits[i].entry);
            out.append(num, (size_t)n);
        }
        append_header(out, c.b, r);
    }
}

static int print_segment(char *to, size_t cap, const char *sep, const kid_segment &s)
{
    return snprintf(to, cap, "%s%u:%u:%u:%u:%u:%u", sep, s.pos, s.n_pos, s.n_kmers, s.n_hits, s.final, s.confident);
}
static int print_segment(char *to, size_t cap, const char *sep, const kid_segment_vote &s)
{
    return snprintf(to, cap, "%s%u:%u:%u:%u:%u:%u:%u:%u", sep, s.pos, s.n_pos, s.n_kmers, s.n_hits, s.call, s.confident, s.p_best, s.n_best);
}
// The segment lines of one classified batch under the rule, for either kind of segment record (print_segment has its
// columns).  A read whose segments hold no hit leaves no line.
template <class Segment, class BlockForm, class OffsetsForm>
static void segment_lines_of(BlockForm block_form, OffsetsForm offsets_form, const Classified &c, const SegmentsOption &o, std::string &out)
{
    const size_t nr = c.b.size();
    std::vector<uint64_t> off(nr + 1);
    const std::vector<Segment> segs = read_items<Segment>(block_form, offsets_form, c.db, c.b, c.bases, o.seg_len, o.seg_step, c.rule().min_hits,
                                                          c.rule().min_permille, off.data());
    if (segs.empty()) return;
    char num[128];
    for (size_t r = 0; r < nr; r++) {
        uint64_t with_hit = 0;
        for (uint64_t i = off[r]; i < off[r + 1]; i++) with_hit += segs[i].n_hits > 0;
        if (with_hit == 0) continue;
        append_head(out, c, r, off[r + 1] - off[r], with_hit);
        const char *sep = "";
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            if (segs[i].n_hits == 0) continue;
            out.append(num, (size_t)print_segment(num, sizeof(num), sep, segs[i]));
            sep = " ";
        }
        append_header(out, c.b, r);
    }
}
static void segments_lines_of(const Classified &c, std::string &out)
{
    segment_lines_of<kid_segment>(kid_db_read_segments_fastq, kid_db_read_segments, c, c.e.side.segments, out);
}
static void segment_votes_lines_of(const Classified &c, std::string &out)
{
    segment_lines_of<kid_segment_vote>(kid_db_read_segment_votes_fastq, kid_db_read_segment_votes, c, c.e.side.segment_votes, out);
}

// The loci records of one classified batch: kid_db_read_loci* with diag_bin = W
static void loci_of(kid_db *db, const ReadBatch &b, const uint8_t *bases, uint32_t diag_bin, std::vector<kid_locus> &loci)
{
    loci.resize(b.size());
    read_pass(kid_db_read_loci_fastq, kid_db_read_loci, db, b, bases, diag_bin, loci.data());
}

// ... under --loci's W, and their lines, with the position of the first entry's probe
static void loci_lines_of(const Classified &c, std::string &out)
{
    if (!c.e.site_pos) return; // (a database without sites)
    loci_of(c.db, c.b, c.bases, c.e.side.loci.diag_bin, c.loci);
    const std::vector<uint32_t> &site_pos = *c.e.site_pos;
    char num[192];
    for (size_t r = 0; r < c.b.size(); r++) {
        const kid_locus &l = c.loci[r];
        if (l.n_hits == 0 || c.dropped(r)) continue;
        const uint32_t at = l.n_chain && l.entry_first < site_pos.size() ? site_pos[l.entry_first] : 0u;
        const int n = snprintf(num, sizeof(num), "%u\t%d\t%u\t%u\t%u:%u:%u:%u:%u:%u:%u:%u", c.final_targ[r], c.b.stop[r] - c.b.start[r] + 1,
                               l.n_kmers, l.n_hits, l.org, l.strand, l.n_chain, l.n_org, l.n_other, l.pos_first, l.pos_last, at);
        out.append(num, (size_t)n);
        append_header(out, c.b, r);
    }
}

// The lines of a run of fragments under --fragment-loci: those with a hit; j0 is the index of the first record in its files
static void fragment_loci_lines(const std::vector<kid_fragment_locus> &recs, unsigned long long j0, std::string &out)
{
    char num[256];
    for (size_t i = 0; i < recs.size(); i++) {
        const kid_fragment_locus &l = recs[i];
        if (l.n_hits == 0) continue;
        const int n = snprintf(num, sizeof(num), "%llu\t%u\t%u\t%u:%u:%u:%u:%u:%u:%u:%u:%u:%u\n", j0 + i, l.n_kmers, l.n_hits, l.org, l.orient, l.mates,
                               l.n_chain, l.n_chain_1, l.n_chain_2, l.n_org, l.n_other, l.lo, l.hi);
        out.append(num, (size_t)n);
    }
}

// (the support pass: nothing comes back, the batch is tallied into the device's confident sample under the rule -- (0, 0)
// when --depth runs it without one)
static void support_into(const Classified &c, kid_sample *tally)
{
    read_pass(kid_db_read_support_fastq, kid_db_read_support, c.db, c.b, c.bases, c.rule().min_hits, c.rule().min_permille, (kid_support *)nullptr, tally);
}
// (the vote pass, under --votes: the batch is tallied into the device's votes sample under the same rule)
static void votes_into(const Classified &c, kid_sample *tally)
{
    read_pass(kid_db_read_votes_fastq, kid_db_read_votes, c.db, c.b, c.bases, c.rule().min_hits, c.rule().min_permille, (kid_vote *)nullptr, tally);
}

// The passes behind the classification of a batch, in the order they run, one call each per batch: the lines of a side file
// that holds one per read (when that file is on), or a tally into the device's sample of a kind (when the engine has it)
static const struct {
    SideFile file;
    void (*lines_of)(const Classified &, std::string &out);
    Tally tally;
    void (*tally_into)(const Classified &, kid_sample *);
} kBatchPasses[] = {{SF_HITS, hit_lines_of, TALLY_COUNT, nullptr},
                    {SF_COUNT, nullptr, TALLY_CONFIDENT, support_into},
                    {SF_COUNT, nullptr, TALLY_VOTES, votes_into},
                    {SF_SEGMENTS, segments_lines_of, TALLY_COUNT, nullptr},
                    {SF_SEGMENT_VOTES, segment_votes_lines_of, TALLY_COUNT, nullptr},
                    {SF_LOCI, loci_lines_of, TALLY_COUNT, nullptr}};

long long run_files(Engine &e, Prefetcher &pf, size_t first, size_t count, ReadSaver &saver, SampleOutputs &out, size_t saver_file,
                    const std::function<void(size_t, long long)> &done)
{
    // Two batches in flight per device: while the GPU classifies batch b, batch b + 1 is uploaded and the results of
    // batch b - 1 go through the read saver -- in file order, which is what decides the "first 12 reads of a target"
    // (newkmer_10nx.cpp:608-612).  FASTQ files arrive as text blocks with a line index (FastqStream): those are trimmed
    // and classified on the GPU (kid_classify_fastq_async); everything else as reads with their range.
    struct InFlight {
        std::unique_ptr<ReadBatch> batch;
        std::vector<uint32_t> final_targ;
        // --low-complexity on a batch of reads (kid_lowc_batch), and in front of it
        // --min-base-quality on a batch of reads with their qualities (a plain FASTQ file, tokenised and trimmed on the
        // host): the copy of the text with the low-quality bases masked (kid_mask_batch) that is classified in its place --
        // the read saver prints the batch's own text
        std::vector<uint8_t> masked;
        const uint8_t *bases() const { return masked.empty() ? batch->bases.data() : masked.data(); }
        HostBuf io;
        uint64_t ticket = 0;
        size_t dev = 0; // the device it was dealt: e.samples[dev] classifies it on e.dbs[dev], the tallies are that device's
        size_t file = 0;
    };
    std::vector<kid_locus> loci;
    std::string lines;
    std::deque<InFlight> q;
    std::vector<long long> handed(count, 0);
    const size_t max_in_flight = 2 * e.samples.size();
    // --fragments, --fragment-votes and --fragment-loci: the blocks of each mate file that are through, in file order, until their records have been paired
    struct HeldBlock {
        std::unique_ptr<ReadBatch> batch;
        size_t paired = 0; // records of the block that have been handed on
    };
    const bool by_fold = out.on(SF_FRAGMENTS) && count == 2 && !e.tallied[TALLY_FRAGMENTS].empty();
    const bool by_votes = out.on(SF_FRAGMENT_VOTES) && count == 2 && !e.tallied[TALLY_FRAGMENT_VOTES].empty();
    const bool by_loci = out.on(SF_FRAGMENT_LOCI) && count == 2 && e.site_pos; // (the databases have their sites: engine_open)
    const bool fragments = by_fold || by_votes || by_loci; // (each pairs the records; all are handed the same run of the same blocks)
    std::vector<kid_fragment_locus> fragment_loci;
    unsigned long long fragments_done = 0; // the index j of the next fragment: the records are paired in file order
    std::deque<HeldBlock> held[2];
    unsigned long long mate_records[2] = {0, 0};
    std::vector<kid_fastq_rec> absent;
    // record j of one file with record j of the other: the longest common run of the two front blocks, until one of the
    // queues is empty; with `flush` (both files are through) what is left of one has absent mates
    auto pair_up = [&](bool flush) {
        for (;;) {
            for (std::deque<HeldBlock> &h : held)
                while (!h.empty() && h.front().paired == h.front().batch->size()) h.pop_front();
            const bool have[2] = {!held[0].empty(), !held[1].empty()};
            if (!have[0] && !have[1]) return;
            if (!(have[0] && have[1]) && !flush) return;
            size_t n = (size_t)-1;
            for (int m = 0; m < 2; m++)
                if (have[m] && held[m].front().batch->size() - held[m].front().paired < n) n = held[m].front().batch->size() - held[m].front().paired;
            if (!(have[0] && have[1])) absent.assign(n, kid_fastq_rec{0, 0, 0, 0});
            const uint8_t *text[2];
            uint64_t nbytes[2];
            const kid_fastq_rec *recs[2];
            for (int m = 0; m < 2; m++) {
                const FastqBlock *fq = have[m] ? held[m].front().batch->fq.get() : nullptr;
                text[m] = fq ? (const uint8_t *)fq->text.data() : nullptr;
                nbytes[m] = fq ? fq->used : 0;
                recs[m] = fq ? fq->recs.data() + held[m].front().paired : absent.data();
            }
            const size_t dev = e.next_fragments;
            e.next_fragments = (e.next_fragments + 1) % e.dbs.size();
            int rc = KID_OK;
            if (by_fold)
                rc = kid_db_read_fragments_fastq(e.dbs[dev], text[0], nbytes[0], recs[0], text[1], nbytes[1], recs[1], n, e.side.support.min_hits,
                                                 e.side.support.min_permille, (kid_fragment *)nullptr, e.tallied[TALLY_FRAGMENTS][dev]);
            if (rc == KID_OK && by_votes)
                rc = kid_db_read_fragment_votes_fastq(e.dbs[dev], text[0], nbytes[0], recs[0], text[1], nbytes[1], recs[1], n,
                                                      e.side.support.min_hits, e.side.support.min_permille, (kid_fragment_vote *)nullptr,
                                                      e.tallied[TALLY_FRAGMENT_VOTES][dev]);
            if (rc == KID_OK && by_loci) {
                fragment_loci.resize(n);
                rc = kid_db_read_fragment_loci_fastq(e.dbs[dev], text[0], nbytes[0], recs[0], text[1], nbytes[1], recs[1], n, e.side.fragment_loci_bin,
                                                     e.side.fragment_loci_span, fragment_loci.data());
                if (rc == KID_OK) {
                    lines.clear();
                    fragment_loci_lines(fragment_loci, fragments_done, lines);
                    out.add(SF_FRAGMENT_LOCI, saver_file, lines);
                }
            }
            if (rc != KID_OK) die_kid(rc);
            fragments_done += n;
            for (int m = 0; m < 2; m++)
                if (have[m]) held[m].front().paired += n;
        }
    };
    const bool pileup_on = out.on(SF_PILEUP) && !e.pileups.empty() && e.site_pos;
    auto retire = [&]() {
        InFlight &f = q.front();
        const auto t0 = std::chrono::steady_clock::now();
        int rc = kid_classify_wait(e.samples[f.dev], f.ticket);
        e.gpu_wait_s += seconds_since(t0);
        if (rc != KID_OK) die_kid(rc);
        if (f.batch->fq) collect_fastq_block(*f.batch, f.io, f.final_targ);
        handed[f.file] += saver.add_batch_of(saver_file + f.file, *f.batch, f.final_targ, e.k);
        const Classified c{e.dbs[f.dev], *f.batch, f.bases(), f.final_targ, e, loci};
        for (const auto &pass : kBatchPasses) {
            if (pass.tally_into) {
                if (!e.tallied[pass.tally].empty()) pass.tally_into(c, e.tallied[pass.tally][f.dev]);
            } else if (out.on(pass.file)) {
                lines.clear();
                pass.lines_of(c, lines);
                out.add(pass.file, saver_file + f.file, lines);
            }
        }
        if (pileup_on) { // one loci pass feeds the loci file and the pileup: --loci's has run, else one with a diagonal bin of 1 runs here
            if (!out.on(SF_LOCI)) loci_of(c.db, c.b, c.bases, 1u, loci);
            if (c.b.fq) { // (the records process_qual drops were never handed to process_read: they have no hit, and do not count)
                size_t kept = 0;
                for (size_t r = 0; r < loci.size(); r++)
                    if (!c.dropped(r)) loci[kept++] = loci[r];
                loci.resize(kept);
            }
            rc = kid_pileup_add(e.pileups[f.dev], loci.data(), loci.size(), e.side.pileup.min_chain, e.side.pileup.min_margin);
            if (rc != KID_OK) die_kid(rc);
        }
        if (fragments && f.batch->fq) {
            mate_records[f.file] += f.batch->size();
            held[f.file].push_back(HeldBlock{std::move(f.batch), 0});
            pair_up(false);
        }
        q.pop_front();
    };
    try {
        for (;;) {
            size_t which = 0;
            std::unique_ptr<ReadBatch> b = pf.next_any(first, first + count, which);
            if (!b) break;
            q.emplace_back();
            InFlight &f = q.back();
            f.batch = std::move(b);
            f.file = which - first;
            const size_t nr = f.batch->size();
            f.dev = e.next_sample; // batches are dealt round-robin over the devices
            e.next_sample = (e.next_sample + 1) % e.samples.size();
            kid_sample *const sample = e.samples[f.dev];
            kid_db *const db = e.dbs[f.dev];
            int rc;
            const auto t_sub = std::chrono::steady_clock::now();
            if (f.batch->fq) {
                rc = submit_fastq_block(sample, *f.batch, f.io, &f.ticket);
            } else {
                f.final_targ.resize(nr);
                rc = KID_OK;
                if (e.side.min_base_quality > 0 && !f.batch->quals.empty()) {
                    f.masked.resize(f.batch->bases.size());
                    rc = kid_mask_batch(db, f.batch->bases.data(), f.batch->quals.data(), f.batch->offsets.data(), nr, e.side.min_base_quality,
                                        f.masked.data(), nullptr);
                }
                if (rc == KID_OK && e.side.low_complexity > 0 && !f.batch->bases.empty()) { // (on what the quality mask left; FASTA too)
                    const bool quality_masked = !f.masked.empty();
                    f.masked.resize(f.batch->bases.size());
                    rc = kid_lowc_batch(db, quality_masked ? f.masked.data() : f.batch->bases.data(), f.batch->offsets.data(), nr,
                                        e.side.low_complexity, f.masked.data(), nullptr);
                }
                if (rc == KID_OK)
                    rc = kid_classify_batch_async(sample, f.bases(), f.batch->offsets.data(), f.batch->start.data(),
                                                  f.batch->stop.data(), nr, f.final_targ.data(), &f.ticket);
            }
            e.submit_s += seconds_since(t_sub);
            if (rc != KID_OK) die_kid(rc);
            while (q.size() > max_in_flight) retire();
        }
    } catch (const Fatal &) {
        // a file failed behind the batches handed out so far: those are the library's until waited for, and the
        // reference had processed them (and every file before the failing one) before it met the failure
        while (!q.empty()) retire();
        throw;
    }
    while (!q.empty()) retire();
    if (fragments) {
        pair_up(true);
        if (mate_records[0] != mate_records[1]) {
            const unsigned long long a = mate_records[0], b = mate_records[1];
            fprintf(stderr, "kmer_id_amd: %s: %s: the mate files hold %llu and %llu records: %llu fragments have an absent mate\n",
                    by_fold ? "--fragments" : by_votes ? "--fragment-votes" : "--fragment-loci", out.result_path().c_str(), a, b, a > b ? a - b : b - a);
        }
    }
    long long n = 0;
    for (size_t f = 0; f < count; f++) {
        saver.file_done(saver_file + f);
        if (done) done(f, handed[f]);
        n += handed[f];
    }
    return n;
}

std::vector<SourceOpener> make_openers(const std::vector<std::string> &paths, int k, std::vector<char> &missing,
                                       std::unique_ptr<ReadSource> (*open)(const std::string &, int, bool *))
{
    missing.assign(paths.size(), 0);
    std::vector<SourceOpener> files;
    for (size_t f = 0; f < paths.size(); f++) {
        const std::string path = paths[f];
        char *flag = &missing[f];
        files.push_back([path, k, flag, open]() {
            bool m = false;
            std::unique_ptr<ReadSource> src = open(path, k, &m);
            *flag = m ? 1 : 0;
            return src;
        });
    }
    return files;
}

static void dry_dump_db(FILE *f, const std::vector<int32_t> &parent, const ProbeSet &ps)
{
    fprintf(f, "PARENT %zu\n", parent.size());
    for (size_t i = 0; i < parent.size(); i++)
        if (parent[i] != 1) fprintf(f, "%zu %d\n", i, parent[i]);
    fprintf(f, "PROBES %zu %lld\n", ps.keys.size(), ps.lines_parsed);
    for (size_t i = 0; i < ps.keys.size(); i++) fprintf(f, "%llu %u\n", (unsigned long long)ps.keys[i], ps.targets[i]);
}

static void dry_dump_source(FILE *f, const std::string &label, ReadSource &src, size_t batch_reads, int k)
{
    ReadBatch b;
    fprintf(f, "FILE %s\n", label.c_str());
    while (src.fill(b, batch_reads, (size_t)-1)) {
        if (b.fq) { // a FASTQ block: what the GPU would do with it (process_qual, the >= k test) done here on the host
            trim_block_on_host(*b.fq, k, b.start, b.stop);
            const char *base = b.fq->text.data();
            for (size_t r = 0; r < b.size(); r++) {
                if (!(b.stop[r] - b.start[r] >= k)) continue;
                fwrite(base + b.fq->acc_off[r], 1, b.fq->acc_len[r], f);
                fprintf(f, "\t%d\t%d\t", b.start[r], b.stop[r]);
                fwrite(base + b.fq->recs[r].seq_off, 1, b.fq->recs[r].seq_len, f);
                fputc('\n', f);
            }
            continue;
        }
        for (size_t r = 0; r < b.size(); r++) {
            fprintf(f, "%s\t%d\t%d\t", b.acc[r].c_str(), b.start[r], b.stop[r]);
            fwrite(b.bases.data() + b.offsets[r], 1, (size_t)(b.offsets[r + 1] - b.offsets[r]), f);
            fputc('\n', f);
        }
    }
    src.close();
}

int write_dry_run(const std::string &path, const char *prog, const std::vector<int32_t> &parent, const ProbeSet &ps,
                  const std::vector<std::string> &labels, const std::vector<SourceOpener> &files, size_t batch_reads, int k)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { perror(prog); return 2; }
    dry_dump_db(f, parent, ps);
    for (size_t i = 0; i < files.size(); i++) {
        std::unique_ptr<ReadSource> src = files[i]();
        if (src) dry_dump_source(f, labels[i], *src, batch_reads, k);
    }
    fclose(f);
    return 0;
}

} // namespace kidhost
