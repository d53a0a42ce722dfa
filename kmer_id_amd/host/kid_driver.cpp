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
    for (const std::vector<kid_sample *> *list : {&samples, &confident, &fragments, &votes, &fragment_votes})
        for (kid_sample *s : *list) kid_sample_destroy(s);
    for (kid_pileup *p : pileups) kid_pileup_destroy(p); // (before their databases)
    if (owns_dbs)
        for (kid_db *d : dbs) kid_db_destroy(d);
}

static kid_sample *begin_sample_or_die(kid_db *db)
{
    kid_sample *s = nullptr;
    int rc = kid_sample_begin(db, &s);
    if (rc != KID_OK) die_kid(rc);
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
    if (side.support.on || side.depth)
        for (kid_db *d : e.dbs) e.confident.push_back(begin_sample_or_die(d));
    if (side.depth)
        for (kid_sample *s : e.confident) {
            int rc = kid_sample_set_option(s, KID_OPT_ENTRY_DEPTH, 1);
            if (rc != KID_OK) die_kid(rc);
        }
    if (side.fragments) // (tallied through the database's hit pass: KID_DB_OPT_MIN_BASE_QUALITY below is what masks for them)
        for (kid_db *d : e.dbs) e.fragments.push_back(begin_sample_or_die(d));
    if (side.votes) // (tallied through the database's hit pass too)
        for (kid_db *d : e.dbs) e.votes.push_back(begin_sample_or_die(d));
    if (side.fragment_votes) // (and so are the fragments called by votes)
        for (kid_db *d : e.dbs) e.fragment_votes.push_back(begin_sample_or_die(d));
    if (side.pileup.on && e.site_pos) // (the databases have their sites: engine_open)
        for (kid_db *d : e.dbs) {
            kid_pileup *p = nullptr;
            int rc = kid_pileup_create(d, side.pileup.bin_width, &p);
            if (rc != KID_OK) die_kid(rc);
            e.pileups.push_back(p);
        }
    // the two masks: the sample's option and the database's, each only where it is on
    const struct { int value, sample_opt, db_opt; } masks[] = {{side.min_base_quality, KID_OPT_MIN_BASE_QUALITY, KID_DB_OPT_MIN_BASE_QUALITY},
                                                               {side.low_complexity, KID_OPT_LOW_COMPLEXITY, KID_DB_OPT_LOW_COMPLEXITY}};
    for (const auto &m : masks) {
        if (m.value == 0) continue;
        for (const std::vector<kid_sample *> *list : {&e.samples, &e.confident})
            for (kid_sample *s : *list) {
                int rc = kid_sample_set_option(s, m.sample_opt, m.value);
                if (rc != KID_OK) die_kid(rc);
            }
        if (!e.owns_dbs) continue; // (a worker: its owner has set it)
        for (kid_db *d : e.dbs) {
            int rc = kid_db_set_option(d, m.db_opt, m.value);
            if (rc != KID_OK) die_kid(rc);
        }
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
    for (const std::vector<kid_sample *> *list : {&e.samples, &e.confident, &e.fragments, &e.votes, &e.fragment_votes})
        for (kid_sample *s : *list) {
            int rc = kid_sample_reset(s);
            if (rc != KID_OK) die_kid(rc);
        }
    for (kid_pileup *p : e.pileups) {
        int rc = kid_pileup_reset(p);
        if (rc != KID_OK) die_kid(rc);
    }
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

[[noreturn]] static void usage_error(const char *prog, const char *option, const char *what)
{
    std::cerr << prog << ": " << option << " " << what << "\n";
    exit(2);
}

// The run of decimal digits at v[at]: its value into `value`, `at` moved behind it.  Returns the number of digits (0: there
// is none), or -1 as soon as the value is above `max`.
static int digits_up_to(unsigned long long max, const char *v, size_t &at, unsigned long long &value)
{
    int n = 0;
    for (value = 0; v[at] >= '0' && v[at] <= '9'; at++, n++) {
        value = value * 10 + (unsigned)(v[at] - '0');
        if (value > max) return -1;
    }
    return n;
}

static void read_min_hits(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    unsigned long long n = 0;
    size_t at = 0;
    const int nd = digits_up_to(0xFFFFFFFFull, v, at, n);
    if (nd < 0) usage_error(prog, opt, "is out of range");
    if (nd == 0 || v[at] != 0) usage_error(prog, opt, "takes a number >= 0");
    o.support.on = true;
    o.support.min_hits = (uint32_t)n;
}

// F -> permille, from its digits: the whole part, then up to three fractional digits padded with zeros
static void read_confidence(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    const char *const what = "takes a decimal in [0, 1], e.g. 0.02";
    unsigned long long whole = 0, frac = 0;
    size_t at = 0;
    const int nd = digits_up_to(0xFFFFFFFFull, v, at, whole);
    if (nd < 0) usage_error(prog, opt, "is out of range");
    if (nd == 0) usage_error(prog, opt, what);
    if (v[at] == '.') {
        const int nfrac = digits_up_to(999, v, ++at, frac);
        if (nfrac < 0 || nfrac > 3) usage_error(prog, opt, "takes at most three fractional digits");
        if (nfrac == 0) usage_error(prog, opt, what);
        for (int j = nfrac; j < 3; j++) frac *= 10;
    }
    if (v[at] != 0) usage_error(prog, opt, what);
    if (whole * 1000 + frac > 1000) usage_error(prog, opt, "takes a decimal in [0, 1]");
    o.support.on = true;
    o.support.min_permille = (uint32_t)(whole * 1000 + frac);
}

static void read_base_quality(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    unsigned long long q = 0;
    size_t at = 0;
    if (digits_up_to(93, v, at, q) <= 0 || v[at] != 0) usage_error(prog, opt, "takes a quality from 0 to 93");
    o.min_base_quality = (int)q;
}

static void read_low_complexity(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    unsigned long long t = 0;
    size_t at = 0;
    if (digits_up_to(1000, v, at, t) <= 0 || v[at] != 0) usage_error(prog, opt, "takes a threshold from 0 to 1000");
    o.low_complexity = (int)t;
}

static SegmentsOption parse_segments(const char *prog, const char *opt, const char *v)
{
    const char *const what = "takes LEN[:STEP], digits only: LEN in 1..2147483647, STEP in 1..LEN with LEN <= 1024 * STEP";
    unsigned long long len = 0, step = 0;
    size_t at = 0;
    if (digits_up_to(0x7FFFFFFFull, v, at, len) <= 0) usage_error(prog, opt, what); // (an empty part too)
    step = len;
    if (v[at] == ':' && digits_up_to(0x7FFFFFFFull, v, ++at, step) <= 0) usage_error(prog, opt, what);
    if (v[at] != 0) usage_error(prog, opt, what); // (a second colon too)
    if (len < 1 || step < 1 || step > len || len > 1024ull * step) usage_error(prog, opt, what);
    return SegmentsOption{true, (uint32_t)len, (uint32_t)step};
}
static void read_segments(SideOptions &o, const char *prog, const char *opt, const char *v) { o.segments = parse_segments(prog, opt, v); }
static void read_segment_votes(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    o.segment_votes = parse_segments(prog, opt, v);
}

static void read_loci(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    unsigned long long w = 0;
    size_t at = 0;
    if (digits_up_to(0x7FFFFFFFull, v, at, w) <= 0 || v[at] != 0 || w < 1) usage_error(prog, opt, "takes W, digits only: 1..2147483647");
    o.loci = LociOption{true, (uint32_t)w};
}

static void read_pileup(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    const char *const what = "takes W[:MIN_CHAIN[:MIN_MARGIN]], digits only: W in 1..2147483647, MIN_CHAIN in 1..4096, MIN_MARGIN in 0..4096";
    unsigned long long w = 0, chain = 2, margin = 1;
    size_t at = 0;
    if (digits_up_to(0x7FFFFFFFull, v, at, w) <= 0) usage_error(prog, opt, what); // (an empty part too)
    if (v[at] == ':' && digits_up_to(4096, v, ++at, chain) <= 0) usage_error(prog, opt, what);
    if (v[at] == ':' && digits_up_to(4096, v, ++at, margin) <= 0) usage_error(prog, opt, what);
    if (v[at] != 0) usage_error(prog, opt, what); // (a fourth part too)
    if (w < 1 || chain < 1) usage_error(prog, opt, what);
    o.pileup = PileupOption{true, (uint32_t)w, (uint32_t)chain, (uint32_t)margin};
}

// The side options: their words, the pass of side_options() that reads each, what reads its value -- or, for a switch,
// which takes none, the flag it sets
static const struct {
    const char *name;
    int pass;
    void (*read)(SideOptions &, const char *prog, const char *opt, const char *v);
    bool SideOptions::*flag;
} kSideOptions[] = {{"--hits", 0, nullptr, &SideOptions::hits},
                    {"--min-hits", 0, read_min_hits, nullptr},
                    {"--confidence", 0, read_confidence, nullptr},
                    {"--min-base-quality", 1, read_base_quality, nullptr},
                    {"--low-complexity", 1, read_low_complexity, nullptr},
                    {"--segments", 2, read_segments, nullptr},
                    {"--segment-votes", 3, read_segment_votes, nullptr},
                    {"--loci", 4, read_loci, nullptr},
                    {"--pileup", 5, read_pileup, nullptr},
                    {"--depth", 0, nullptr, &SideOptions::depth},
                    {"--seen", 0, nullptr, &SideOptions::seen},
                    {"--fragments", 0, nullptr, &SideOptions::fragments},
                    {"--votes", 0, nullptr, &SideOptions::votes},
                    {"--fragment-votes", 0, nullptr, &SideOptions::fragment_votes}};

int side_option_values(const char *word)
{
    for (const auto &so : kSideOptions)
        if (strcmp(word, so.name) == 0) return so.read ? 1 : 0;
    return -1;
}

SideOptions side_options(int argc, char **argv, const char *prog)
{
    SideOptions o;
    // one pass over the words per step of the order in which malformed options are reported
    for (int pass = 0; pass < 6; pass++)
        for (int i = 1; i < argc; i++)
            for (const auto &so : kSideOptions) {
                if (so.pass != pass || strcmp(argv[i], so.name) != 0) continue;
                if (!so.read) { o.*so.flag = true; continue; }
                if (i + 1 >= argc) usage_error(prog, so.name, "needs a value");
                so.read(o, prog, so.name, argv[i + 1]);
            }
    return o;
}

// The file beside a result file: its path with the last "result" replaced by `word`
static std::string sibling_path_for(const std::string &result_path, const char *word)
{
    std::string p = result_path;
    const size_t at = p.rfind("result");
    if (at != std::string::npos) p.replace(at, 6, word);
    return p;
}

// The side files beside a result file: the one place that has their names
struct SidePaths { std::string hits, confident, segments, depth, seen, fragments, votes, fragment_votes, segment_votes, loci, pileup; };
static SidePaths side_paths(const std::string &r)
{
    std::string seen = r; // the final "result.txt" becomes "seen.bin"
    const size_t at = seen.rfind("result.txt");
    if (at != std::string::npos) seen.replace(at, 10, "seen.bin");
    else seen += ".seen.bin";
    return {sibling_path_for(r, "hits"), sibling_path_for(r, "confident"), sibling_path_for(r, "segments"), sibling_path_for(r, "depth"), seen,
            sibling_path_for(r, "fragments"), sibling_path_for(r, "votes"), sibling_path_for(r, "fragment_votes"), sibling_path_for(r, "segment_votes"),
            sibling_path_for(r, "loci"), sibling_path_for(r, "pileup")};
}

void remove_side_files(const std::string &result_path, const SideOptions &side, bool all)
{
    const SidePaths p = side_paths(result_path);
    if (all || side.hits) remove(p.hits.c_str());
    if (all || side.segments.on) remove(p.segments.c_str());
    if (all || side.support.on) remove(p.confident.c_str());
    if (all || side.depth) remove(p.depth.c_str());
    if (all || side.seen) remove(p.seen.c_str());
    if (all || side.fragments) remove(p.fragments.c_str());
    if (all || side.votes) remove(p.votes.c_str());
    if (all || side.fragment_votes) remove(p.fragment_votes.c_str());
    if (all || side.segment_votes.on) remove(p.segment_votes.c_str());
    if (all || side.loci.on) remove(p.loci.c_str());
    if (all || side.pileup.on) remove(p.pileup.c_str());
}

SampleOutputs::SampleOutputs(const std::string &result_path, const SideOptions &side) : side_(side), result_path_(result_path)
{
    remove_side_files(result_path, side);
}

void SampleOutputs::add(Lines &to, size_t file, const std::string &lines)
{
    if (to.size() <= file) to.resize(file + 1);
    to[file] += lines;
}

static void write_lines(const std::string &path, const std::vector<std::string> &parts)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) throw Fatal{2, "cannot write " + path};
    for (const std::string &p : parts) fwrite(p.data(), 1, p.size(), f);
    fclose(f);
}

// gcount / ucount of a sample (one per device, merged) -> "<i>,<g>,<u>" lines
static void write_counters(std::vector<kid_sample *> &samples, int ntar, const std::string &path)
{
    std::vector<int64_t> g((size_t)ntar), u((size_t)ntar);
    int rc = samples.size() > 1 ? kid_sample_end_merged(samples.data(), (int)samples.size(), g.data(), u.data())
                                : kid_sample_end(samples[0], g.data(), u.data());
    if (rc != KID_OK) die_kid(rc);
    write_result(path, g, u);
}

// The depth spectrum (256 bins) of the tallied sample (one per device, merged) -> "<i>,<kmer_hits>,<distinct>,<q1>,<q2>,<q3>,<max>"
// lines: distinct = the target's entries with a hit; q_p = the smallest depth d >= 1 with 4 * #{entries: 1 <= depth <= d}
// >= p * distinct, the last column taken as d = 255; 0 without a hit
static void write_depth(std::vector<kid_sample *> &samples, int ntar, const std::string &path)
{
    const uint32_t bins = 256;
    std::vector<uint64_t> spectrum((size_t)ntar * bins), ksum((size_t)ntar);
    std::vector<uint32_t> dmax((size_t)ntar);
    int rc = kid_sample_depth_spectrum_merged(samples.data(), (int)samples.size(), bins, spectrum.data(), ksum.data(), dmax.data());
    if (rc != KID_OK) die_kid(rc);
    std::string text;
    char line[160];
    for (int i = 0; i < ntar; i++) {
        const uint64_t *row = &spectrum[(size_t)i * bins];
        uint64_t distinct = 0, below = 0;
        for (uint32_t d = 1; d < bins; d++) distinct += row[d];
        uint32_t q[3] = {0, 0, 0};
        int p = 0;
        for (uint32_t d = 1; d < bins && p < 3 && distinct; d++) {
            below += row[d];
            while (p < 3 && 4 * below >= (uint64_t)(p + 1) * distinct) q[p++] = d;
        }
        const int n = snprintf(line, sizeof(line), "%d,%llu,%llu,%u,%u,%u,%u\n", i, (unsigned long long)ksum[(size_t)i],
                               (unsigned long long)distinct, q[0], q[1], q[2], dmax[(size_t)i]);
        text.append(line, (size_t)n);
    }
    write_lines(path, std::vector<std::string>(1, text));
}

const char kSeenMagic[9] = "KIDSEEN1";

// The bitmap of a sample that has been closed (with several devices the first one's holds the union: kid_sample_end_merged)
// -> a seen file
static void write_seen(kid_sample *s, const Engine &e, const std::string &path)
{
    kid_db_info info;
    uint64_t nbytes = 0;
    int rc = kid_db_get_info(e.db, &info);
    if (rc == KID_OK) rc = kid_sample_seen_bytes(s, &nbytes);
    if (rc != KID_OK) die_kid(rc);
    std::vector<uint8_t> bitmap(nbytes);
    if ((rc = kid_sample_seen_export(s, 0, nbytes, bitmap.data(), 0)) != KID_OK) die_kid(rc);
    const uint64_t n_entries = info.n_entries;
    const int32_t ntar = e.ntar, k = e.k;
    char head[32];
    memcpy(head, kSeenMagic, 8);
    memcpy(head + 8, &n_entries, 8);
    memcpy(head + 16, &ntar, 4);
    memcpy(head + 20, &k, 4);
    memcpy(head + 24, &nbytes, 8);
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw Fatal{2, "cannot write " + path};
    const bool ok = fwrite(head, 1, 32, f) == 32 && fwrite(bitmap.data(), 1, bitmap.size(), f) == bitmap.size();
    if (fclose(f) != 0 || !ok) {
        remove(path.c_str());
        throw Fatal{2, "cannot write " + path};
    }
}

int read_seen_files(const std::vector<std::string> &paths, long long ntar, unsigned long long k, std::vector<std::vector<uint8_t>> &maps,
                    SeenHeader &first, std::string &what)
{
    auto fail = [&](int code, const std::string &w) { what = w; return code; };
    const size_t n = paths.size();
    maps.assign(n, std::vector<uint8_t>());
    for (size_t f = 0; f < n; f++) {
        FILE *in = fopen(paths[f].c_str(), "rb");
        if (!in) return fail(255, "cannot open " + paths[f]);
        char head[32];
        SeenHeader h;
        const bool have_head = fread(head, 1, 32, in) == 32;
        if (have_head && memcmp(head, kSeenMagic, 8) == 0) {
            memcpy(&h.n_entries, head + 8, 8);
            memcpy(&h.ntar, head + 16, 4);
            memcpy(&h.k, head + 20, 4);
            memcpy(&h.nbytes, head + 24, 8);
        }
        const uint64_t want = h.n_entries < 0xFFFFFFFFull ? (h.n_entries ? (h.n_entries + 127) / 128 * 16 : 16) : 0;
        bool whole = false;
        if (have_head && h.nbytes == want && want) {
            maps[f].resize(want);
            whole = fread(maps[f].data(), 1, want, in) == want && fgetc(in) == EOF;
        }
        fclose(in);
        if (!have_head) return fail(3, paths[f] + " is truncated: it has no whole header");
        if (memcmp(head, kSeenMagic, 8) != 0) return fail(3, paths[f] + " is not a seen file (bad magic)");
        if (h.nbytes != want || !want) return fail(3, paths[f] + ": the size of its bitmap does not fit its number of entries");
        if (!whole) return fail(3, paths[f] + " is truncated, or has bytes behind its bitmap");
        if (f == 0) first = h;
        if (h.n_entries != first.n_entries || h.ntar != first.ntar || h.k != first.k)
            return fail(3, paths[f] + " was written for another database than " + paths[0] + " (entries, targets or k differ)");
        if (ntar >= 0 && ((unsigned long long)h.ntar != (unsigned long long)ntar || (unsigned long long)h.k != k))
            return fail(3, paths[f] + " was written with --ntar " + std::to_string(h.ntar) + " --k " + std::to_string(h.k) +
                               ", not " + std::to_string(ntar) + " and " + std::to_string(k));
        if (ntar < 0 && (unsigned long long)h.k != k)
            return fail(3, paths[f] + " was written with --k " + std::to_string(h.k) + ", not " + std::to_string(k));
    }
    return 0;
}

// The pileups of a sample (one per device: the others are merged into the first) -> the head line and one line per
// organism with a placed read
static void write_pileup(std::vector<kid_pileup *> &pileups, const PileupOption &o, const std::string &path)
{
    kid_pileup *all = pileups[0];
    uint32_t n_orgs = 0;
    uint64_t n_bins = 0;
    int rc = kid_pileup_info(all, &n_orgs, &n_bins, nullptr);
    if (rc != KID_OK) die_kid(rc);
    if (pileups.size() > 1) {
        std::vector<uint32_t> starts((size_t)n_bins + 1), steps((size_t)n_bins + n_orgs + 1);
        for (size_t i = 1; i < pileups.size(); i++) {
            uint64_t n_records = 0, n_placed = 0;
            if ((rc = kid_pileup_export(pileups[i], starts.data(), steps.data())) != KID_OK) die_kid(rc);
            if ((rc = kid_pileup_counts(pileups[i], &n_records, &n_placed)) != KID_OK) die_kid(rc);
            if ((rc = kid_pileup_merge(all, starts.data(), steps.data(), n_records, n_placed)) != KID_OK) die_kid(rc);
        }
    }
    uint64_t n_records = 0, n_placed = 0;
    std::vector<kid_pileup_rec> recs((size_t)n_orgs + 1);
    if ((rc = kid_pileup_counts(all, &n_records, &n_placed)) != KID_OK) die_kid(rc);
    if ((rc = kid_pileup_summary(all, recs.data())) != KID_OK) die_kid(rc);
    std::string text;
    char line[256];
    int n = snprintf(line, sizeof(line), "#%llu,%llu,%u,%u,%u\n", (unsigned long long)n_records, (unsigned long long)n_placed, o.bin_width,
                     o.min_chain, o.min_margin);
    text.append(line, (size_t)n);
    for (uint32_t g = 0; g < n_orgs; g++) {
        const kid_pileup_rec &r = recs[g];
        if (r.n_placed == 0) continue;
        n = snprintf(line, sizeof(line), "%u,%u,%u,%u,%u,%u,%u,%u,%u,%llu\n", g, r.n_placed, r.span_bins, r.bins_covered, r.max_gap, r.max_depth,
                     r.max_depth_bin, r.max_starts, r.max_starts_bin, (unsigned long long)r.depth_sum);
        text.append(line, (size_t)n);
    }
    write_lines(path, std::vector<std::string>(1, text));
}

void SampleOutputs::finish(Engine &e)
{
    const SidePaths p = side_paths(result_path_);
    write_counters(e.samples, e.ntar, result_path_);
    if (side_.support.on) write_counters(e.confident, e.ntar, p.confident);
    if (side_.fragments) write_counters(e.fragments, e.ntar, p.fragments);
    if (side_.votes) write_counters(e.votes, e.ntar, p.votes);
    if (side_.fragment_votes) write_counters(e.fragment_votes, e.ntar, p.fragment_votes);
    if (side_.depth) write_depth(e.confident, e.ntar, p.depth);
    if (side_.seen) write_seen(side_.support.on ? e.confident[0] : e.samples[0], e, p.seen);
    if (side_.hits) write_lines(p.hits, hits_);
    if (side_.segments.on) write_lines(p.segments, segments_);
    if (side_.segment_votes.on) write_lines(p.segment_votes, segment_votes_);
    if (side_.loci.on) write_lines(p.loci, loci_);
    if (side_.pileup.on && !e.pileups.empty()) write_pileup(e.pileups, side_.pileup, p.pileup);
    hits_.clear();
    segments_.clear();
    segment_votes_.clear();
    loci_.clear();
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
// The end of a read's line: its header line as in _reads.txt
static void append_header(std::string &out, const ReadBatch &b, size_t r)
{
    out += '\t';
    if (b.fq) out.append(b.fq->text.data() + b.fq->acc_off[r], b.fq->acc_len[r]);
    else out += b.acc[r];
    out += '\n';
}

// The hit lines of one classified batch: kid_db_read_hits*
static void hit_lines_of(kid_db *db, const ReadBatch &b, const uint8_t *bases, const std::vector<uint32_t> &final_targ, int k, std::string &out)
{
    const size_t nr = b.size();
    std::vector<uint64_t> off(nr + 1);
    std::vector<uint32_t> nk(nr);
    const std::vector<kid_hit> hits = read_items<kid_hit>(kid_db_read_hits_fastq, kid_db_read_hits, db, b, bases, off.data(), nk.data());
    if (hits.empty()) return;
    char num[64];
    for (size_t r = 0; r < nr; r++) {
        if (off[r + 1] == off[r]) continue;
        if (b.fq && !(b.stop[r] - b.start[r] >= k)) continue; // (dropped by process_qual: it has no hits anyway)
        int n = snprintf(num, sizeof(num), "%u\t%d\t%u\t%llu\t", final_targ[r], b.stop[r] - b.start[r] + 1, nk[r],
                         (unsigned long long)(off[r + 1] - off[r]));
        out.append(num, (size_t)n);
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            n = snprintf(num, sizeof(num), "%s%u:%u:%u", i > off[r] ? " " : "", hits[i].pos, hits[i].target, hits[i].entry);
            out.append(num, (size_t)n);
        }
        append_header(out, b, r);
    }
}

// The segment lines of one classified batch: kid_db_read_segments* under the rule.  A read whose segments hold no hit
// leaves no line.
static void segment_lines_of(kid_db *db, const ReadBatch &b, const uint8_t *bases, const std::vector<uint32_t> &final_targ,
                             const SegmentsOption &o, const SupportRule &rule, std::string &out)
{
    const size_t nr = b.size();
    std::vector<uint64_t> off(nr + 1);
    const std::vector<kid_segment> segs = read_items<kid_segment>(kid_db_read_segments_fastq, kid_db_read_segments, db, b, bases, o.seg_len,
                                                                  o.seg_step, rule.min_hits, rule.min_permille, off.data());
    if (segs.empty()) return;
    char num[96];
    for (size_t r = 0; r < nr; r++) {
        uint64_t with_hit = 0;
        for (uint64_t i = off[r]; i < off[r + 1]; i++) with_hit += segs[i].n_hits > 0;
        if (with_hit == 0) continue;
        int n = snprintf(num, sizeof(num), "%u\t%d\t%llu\t%llu\t", final_targ[r], b.stop[r] - b.start[r] + 1,
                         (unsigned long long)(off[r + 1] - off[r]), (unsigned long long)with_hit);
        out.append(num, (size_t)n);
        bool first = true;
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            const kid_segment &s = segs[i];
            if (s.n_hits == 0) continue;
            n = snprintf(num, sizeof(num), "%s%u:%u:%u:%u:%u:%u", first ? "" : " ", s.pos, s.n_pos, s.n_kmers, s.n_hits, s.final, s.confident);
            out.append(num, (size_t)n);
            first = false;
        }
        append_header(out, b, r);
    }
}

// The segment_votes lines of one classified batch: kid_db_read_segment_votes* under the rule, as segment_lines_of
static void segment_vote_lines_of(kid_db *db, const ReadBatch &b, const uint8_t *bases, const std::vector<uint32_t> &final_targ,
                                  const SegmentsOption &o, const SupportRule &rule, std::string &out)
{
    const size_t nr = b.size();
    std::vector<uint64_t> off(nr + 1);
    const std::vector<kid_segment_vote> segs = read_items<kid_segment_vote>(kid_db_read_segment_votes_fastq, kid_db_read_segment_votes, db, b,
                                                                            bases, o.seg_len, o.seg_step, rule.min_hits, rule.min_permille,
                                                                            off.data());
    if (segs.empty()) return;
    char num[128];
    for (size_t r = 0; r < nr; r++) {
        uint64_t with_hit = 0;
        for (uint64_t i = off[r]; i < off[r + 1]; i++) with_hit += segs[i].n_hits > 0;
        if (with_hit == 0) continue;
        int n = snprintf(num, sizeof(num), "%u\t%d\t%llu\t%llu\t", final_targ[r], b.stop[r] - b.start[r] + 1,
                         (unsigned long long)(off[r + 1] - off[r]), (unsigned long long)with_hit);
        out.append(num, (size_t)n);
        bool first = true;
        for (uint64_t i = off[r]; i < off[r + 1]; i++) {
            const kid_segment_vote &s = segs[i];
            if (s.n_hits == 0) continue;
            n = snprintf(num, sizeof(num), "%s%u:%u:%u:%u:%u:%u:%u:%u", first ? "" : " ", s.pos, s.n_pos, s.n_kmers, s.n_hits, s.call, s.confident,
                         s.p_best, s.n_best);
            out.append(num, (size_t)n);
            first = false;
        }
        append_header(out, b, r);
    }
}

// The loci records of one classified batch: kid_db_read_loci* with diag_bin = W
static void loci_of(kid_db *db, const ReadBatch &b, const uint8_t *bases, uint32_t diag_bin, std::vector<kid_locus> &loci)
{
    loci.resize(b.size());
    read_pass(kid_db_read_loci_fastq, kid_db_read_loci, db, b, bases, diag_bin, loci.data());
}

// ... and their lines; site_pos: the position of every entry's probe
static void loci_lines_of(const std::vector<kid_locus> &loci, const ReadBatch &b, const std::vector<uint32_t> &final_targ, int k,
                          const std::vector<uint32_t> &site_pos, std::string &out)
{
    const size_t nr = b.size();
    char num[192];
    for (size_t r = 0; r < nr; r++) {
        const kid_locus &l = loci[r];
        if (l.n_hits == 0) continue;
        if (b.fq && !(b.stop[r] - b.start[r] >= k)) continue; // (dropped by process_qual: it has no hits anyway)
        const uint32_t at = l.n_chain && l.entry_first < site_pos.size() ? site_pos[l.entry_first] : 0u;
        const int n = snprintf(num, sizeof(num), "%u\t%d\t%u\t%u\t%u:%u:%u:%u:%u:%u:%u:%u", final_targ[r], b.stop[r] - b.start[r] + 1, l.n_kmers,
                               l.n_hits, l.org, l.strand, l.n_chain, l.n_org, l.n_other, l.pos_first, l.pos_last, at);
        out.append(num, (size_t)n);
        append_header(out, b, r);
    }
}

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
        kid_sample *sample = nullptr;
        kid_db *db = nullptr;
        kid_sample *confident = nullptr;
        kid_sample *votes = nullptr;
        kid_pileup *pileup = nullptr;
        size_t file = 0;
    };
    std::vector<kid_locus> loci;
    std::string lines;
    std::deque<InFlight> q;
    std::vector<long long> handed(count, 0);
    const size_t max_in_flight = 2 * e.samples.size();
    // --fragments and --fragment-votes: the blocks of each mate file that are through, in file order, until their records have been paired
    struct HeldBlock {
        std::unique_ptr<ReadBatch> batch;
        size_t paired = 0; // records of the block that have been handed on
    };
    const bool by_fold = out.fragments_on() && count == 2 && !e.fragments.empty();
    const bool by_votes = out.fragment_votes_on() && count == 2 && !e.fragment_votes.empty();
    const bool fragments = by_fold || by_votes; // (either pairs the records; both are handed the same run of the same blocks)
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
                                                 e.side.support.min_permille, (kid_fragment *)nullptr, e.fragments[dev]);
            if (rc == KID_OK && by_votes)
                rc = kid_db_read_fragment_votes_fastq(e.dbs[dev], text[0], nbytes[0], recs[0], text[1], nbytes[1], recs[1], n,
                                                      e.side.support.min_hits, e.side.support.min_permille, (kid_fragment_vote *)nullptr,
                                                      e.fragment_votes[dev]);
            if (rc != KID_OK) die_kid(rc);
            for (int m = 0; m < 2; m++)
                if (have[m]) held[m].front().paired += n;
        }
    };
    auto retire = [&]() {
        InFlight &f = q.front();
        const auto t0 = std::chrono::steady_clock::now();
        int rc = kid_classify_wait(f.sample, f.ticket);
        e.gpu_wait_s += seconds_since(t0);
        if (rc != KID_OK) die_kid(rc);
        if (f.batch->fq) collect_fastq_block(*f.batch, f.io, f.final_targ);
        handed[f.file] += saver.add_batch_of(saver_file + f.file, *f.batch, f.final_targ, e.k);
        if (out.hits_on()) {
            lines.clear();
            hit_lines_of(f.db, *f.batch, f.bases(), f.final_targ, e.k, lines);
            out.add_hits(saver_file + f.file, lines);
        }
        // (the support pass: nothing comes back, the batch is tallied into the device's confident sample under the rule --
        // (0, 0) when --depth runs it without one)
        if (f.confident)
            read_pass(kid_db_read_support_fastq, kid_db_read_support, f.db, *f.batch, f.bases(), e.side.support.min_hits,
                      e.side.support.min_permille, (kid_support *)nullptr, f.confident);
        // (the vote pass, under --votes: the batch is tallied into the device's votes sample under the same rule)
        if (f.votes)
            read_pass(kid_db_read_votes_fastq, kid_db_read_votes, f.db, *f.batch, f.bases(), e.side.support.min_hits, e.side.support.min_permille,
                      (kid_vote *)nullptr, f.votes);
        if (out.segments_on()) {
            lines.clear();
            segment_lines_of(f.db, *f.batch, f.bases(), f.final_targ, e.side.segments, e.side.support, lines);
            out.add_segments(saver_file + f.file, lines);
        }
        if (out.segment_votes_on()) {
            lines.clear();
            segment_vote_lines_of(f.db, *f.batch, f.bases(), f.final_targ, e.side.segment_votes, e.side.support, lines);
            out.add_segment_votes(saver_file + f.file, lines);
        }
        if ((out.loci_on() || f.pileup) && e.site_pos) { // one loci pass feeds both: --loci's diagonal bin when given, else 1
            loci_of(f.db, *f.batch, f.bases(), out.loci_on() ? e.side.loci.diag_bin : 1u, loci);
            if (out.loci_on()) {
                lines.clear();
                loci_lines_of(loci, *f.batch, f.final_targ, e.k, *e.site_pos, lines);
                out.add_loci(saver_file + f.file, lines);
            }
            if (f.pileup) {
                if (f.batch->fq) { // (the records process_qual drops were never handed to process_read: they have no hit, and do not count)
                    size_t kept = 0;
                    for (size_t r = 0; r < loci.size(); r++)
                        if (f.batch->stop[r] - f.batch->start[r] >= e.k) loci[kept++] = loci[r];
                    loci.resize(kept);
                }
                int rc = kid_pileup_add(f.pileup, loci.data(), loci.size(), e.side.pileup.min_chain, e.side.pileup.min_margin);
                if (rc != KID_OK) die_kid(rc);
            }
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
            f.sample = e.samples[e.next_sample]; // batches are dealt round-robin over the devices
            f.db = e.dbs[e.next_sample];
            f.confident = e.confident.empty() ? nullptr : e.confident[e.next_sample];
            f.votes = e.votes.empty() ? nullptr : e.votes[e.next_sample];
            f.pileup = out.pileup_on() && !e.pileups.empty() ? e.pileups[e.next_sample] : nullptr;
            e.next_sample = (e.next_sample + 1) % e.samples.size();
            int rc;
            const auto t_sub = std::chrono::steady_clock::now();
            if (f.batch->fq) {
                rc = submit_fastq_block(f.sample, *f.batch, f.io, &f.ticket);
            } else {
                f.final_targ.resize(nr);
                rc = KID_OK;
                if (e.side.min_base_quality > 0 && !f.batch->quals.empty()) {
                    f.masked.resize(f.batch->bases.size());
                    rc = kid_mask_batch(f.db, f.batch->bases.data(), f.batch->quals.data(), f.batch->offsets.data(), nr, e.side.min_base_quality,
                                        f.masked.data(), nullptr);
                }
                if (rc == KID_OK && e.side.low_complexity > 0 && !f.batch->bases.empty()) { // (on what the quality mask left; FASTA too)
                    const bool quality_masked = !f.masked.empty();
                    f.masked.resize(f.batch->bases.size());
                    rc = kid_lowc_batch(f.db, quality_masked ? f.masked.data() : f.batch->bases.data(), f.batch->offsets.data(), nr,
                                        e.side.low_complexity, f.masked.data(), nullptr);
                }
                if (rc == KID_OK)
                    rc = kid_classify_batch_async(f.sample, f.bases(), f.batch->offsets.data(), f.batch->start.data(),
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
                    by_fold ? "--fragments" : "--fragment-votes", out.result_path().c_str(), a, b, a > b ? a - b : b - a);
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

ReaderOptions parse_reader_options(int argc, char **argv, int default_threads)
{
    ReaderOptions o;
    o.threads = default_threads;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : "";
        if (a == "--k") o.k = atoi(v);
        if (a == "--log2-slots") o.log2_slots = atoi(v);
        if (a == "--device") o.device = atoi(v);
        if (a == "--devices") o.device_list = v;
        if (a == "--batch-reads") o.batch_reads = (size_t)atoll(v);
        if (a == "--dry-run") o.dry_run = v;
        if (a == "--threads") o.threads = atoi(v);
        if (a == "--db-cache") o.db_cache = v;
    }
    o.side = side_options(argc, argv, argv[0]);
    if (o.side.fragments) usage_error(argv[0], "--fragments", "is an option of nk10 alone: the inputs of this program are read one file after the other");
    if (o.side.fragment_votes)
        usage_error(argv[0], "--fragment-votes", "is an option of nk10 alone: the inputs of this program are read one file after the other");
    return o;
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
