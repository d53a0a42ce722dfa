// kid_driver.h -- what the three front-ends (nk10, kmer_read_vf6, kmer_read_m3) share: the database
// on the GPU, the reader-thread / GPU-thread pipeline over the input files, closing a sample.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "kid_host.h"
#include "kid_side.h"
#include "kmer_id_amd.h"

namespace kidhost {

struct Engine {
    kid_db *db = nullptr;         // the database on the first device
    kid_sample *sample = nullptr; // ... and its sample
    // one replica of the database + one sample per device (--devices a,b,...): [0] are the two above.  The batches of
    // a file are dealt round-robin over the samples, the per-read results come back in file order, and closing a
    // sample merges the replicas' counters (kid_sample_end_merged).
    std::vector<kid_db *> dbs;
    std::vector<kid_sample *> samples;
    size_t next_sample = 0;
    // the side options (engine_configure) and what they add per device: the tallied samples that kTallies wants under
    // them, dealt and reset with the classified ones
    SideOptions side;
    std::vector<kid_sample *> tallied[TALLY_COUNT];
    size_t next_fragments = 0; // the fragments are dealt round-robin over the devices on their own
    // under --loci: the position of every entry's probe (the host's copy of what the replicas got in engine_open: the loci
    // file prints pos[entry_first]); a worker shares its owner's
    std::shared_ptr<const std::vector<uint32_t>> site_pos;
    // under --pileup: one pileup per device (engine_configure), reset with the samples, merged into [0] when a sample is closed
    std::vector<kid_pileup *> pileups;
    int ntar = 0, k = 30;
    size_t batch_reads = 1 << 20;
    size_t batch_bases = 256u << 20;
    double gpu_wait_s = 0, submit_s = 0; // the consumer, inside kid_classify_wait / kid_classify_*_async (--timing)
    bool owns_dbs = true; // false: a worker of engine_worker() -- its own samples on the owner's databases
    ~Engine();
};
// Another set of samples (one per device) on the databases of `owner`: for a thread that classifies another input
// sample at the same time (nk10 --samples-in-flight).  The owner must outlive it.
std::unique_ptr<Engine> engine_worker(const Engine &owner);

// The library's error, then leave_now() with the reference's exit code: 1 for a full table, 134 for a malformed record, else 3
[[noreturn]] void die_kid(int rc);
// The end of a front-end that has written everything: flush the standard streams and leave without unwinding -- giving
// page-locked buffers, device memory and the HIP runtime back one by one takes 0.15 s that the operating system does at once.
[[noreturn]] void leave_now(int exit_code);

// tree + probes, from the binary cache when `cache_path` names a valid one, else from the text files
// (and the cache is written for the next run).  `from_cache` reports which way it went.
// `threads`: parse workers of the probes text (0: one per core, at most 8).  `cache_writer`: if given, a cache that has
// to be (re)written is written on that thread -- join it before `parent` / `ps` go away.
// `want_sites` (--loci, --pileup): ps.orgs / ps.positions are filled as well.  The cache does not hold them and its format does not
// change: behind a valid cache the probes text is still read once, for the sites alone (its entries must be the cache's).
void load_database(const std::string &tree_path, const std::string &probes_path, const std::string &cache_path, int k, int ntar,
                   std::vector<int32_t> &parent, ProbeSet &ps, bool *from_cache = nullptr, int threads = 0,
                   StartupTiming *timing = nullptr, std::thread *cache_writer = nullptr, bool want_sites = false);

// Hashtable + Tree1 onto the GPU(s) of parse_devices(): the table is built on the first device and replicated into the
// others.  A ProbeSet with sites (--loci, --pileup): every replica gets them (kid_db_set_sites) and e.site_pos a copy of the
// positions.  Returns false after printing the reference's "out of memory in table " (newkmer_10nx.cpp:256-260: the caller
// exits with 1).
bool engine_open(Engine &e, const ProbeSet &ps, const std::vector<int32_t> &parent, int k, int log2_slots, int max_probes,
                 unsigned flags, const std::vector<int> &devices);
// The side options for an engine that is open: the tallied samples of kTallies (--depth switches the depth counters of the
// confident ones on), under --pileup one pileup per device (the sites are there: engine_open), then --min-base-quality and
// --low-complexity on every replica of the database and on the samples that take them.  A worker of engine_worker()
// inherits them for its samples.
void engine_configure(Engine &e, const SideOptions &side);
// --device D / --devices A,B,... ("0,1,2,3"; a device may be named twice): the list when there is one, else D
std::vector<int> parse_devices(int device, const std::string &list);
// newkmer_10nx.cpp:1017-1019 on every replica
void engine_reset(Engine &e);

// The input files of a run, parsed (+ trimmed) ahead of their turn on a small pool of reader threads:
// gzip inflate + parsing is the slow half of the program (~1 M reads/s per core) and files are
// independent until their reads reach the counters.  Batches are handed out strictly in file order;
// a reader that runs ahead blocks once its file has `depth` batches queued, so memory stays bounded.
// A failure while reading file i surfaces when the consumer gets to file i (the files before it have
// been processed completely, like in the sequential reference).
using SourceOpener = std::function<std::unique_ptr<ReadSource>()>;
class Prefetcher {
public:
    Prefetcher(std::vector<SourceOpener> files, int threads, size_t batch_reads, size_t batch_bases, size_t depth = 3);
    ~Prefetcher();
    // next batch of ANY of the files [lo, hi) -- whichever has one ready; `which` says whose.  nullptr when all of them
    // are at their end.  A file that failed throws its Fatal only once the files before it in the range are through
    // (the reference would have read those completely before it met the failure).
    std::unique_ptr<ReadBatch> next_any(size_t lo, size_t hi, size_t &which);
    SourceStats file_stats(size_t index); // of a file that is through
    double seconds_waited() const;        // the consumer, inside next_any(): the host stages were the slower side
private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// Classify the files [first, first + count) of ONE sample, read at the same time (the two mates of nk10: two inflate
// threads instead of one after the other); the counters do not care about the order, the read saver restores it.
// `saver_file` is the saver's index of file `first` (a saver may span several calls: the files of a kmer_read_vf6 job,
// -f1 and -f2 of kmer_read_m3).  done(f, handed), if given, is called for every file first + f in file order once all of
// them are through, with the number of its reads handed to process_read.  Returns the reads handed of all the files.
// The passes behind the classification of a batch run on the device that classified it, once its final targets are back:
// the support pass (kid_db_read_support*) under e.side.support or e.side.depth and the vote pass (kid_db_read_votes*)
// under e.side.votes, each into that device's tallied sample; one pass per side file of lines that is on in `out`, which
// receives its lines; the loci pass once for the loci file and the device's pileup.
// With the fragments or fragment_votes file on and count == 2 the two files are the mates of a sample: the FASTQ blocks of
// each that are through wait in a queue until the partner's records have arrived; the longest common run of records is
// handed to kid_db_read_fragments_fastq with a device's fragment sample as its tally (and, or, to
// kid_db_read_fragment_votes_fastq with that device's fragment_votes sample: the same run of the same blocks), and a
// block goes as soon as its last record has: none is held longer than the other file lags.
long long run_files(Engine &e, Prefetcher &pf, size_t first, size_t count, ReadSaver &saver, SampleOutputs &out, size_t saver_file = 0,
                    const std::function<void(size_t, long long)> &done = nullptr);

// One opener per path, each by `open`, which sets its bool when the file is a plain FASTA that is not there (the
// reference's "nark <name>"): missing[f] holds it for file f once that file is through.  `missing` must not move
// while the files are read.
std::vector<SourceOpener> make_openers(const std::vector<std::string> &paths, int k, std::vector<char> &missing,
                                       std::unique_ptr<ReadSource> (*open)(const std::string &, int, bool *) = open_by_suffix);

// --dry-run FILE (host stages only, no GPU): the database and the reads of `files` as they WOULD be handed to the GPU, as
// text, each file under its label (a file without a reader is left out).  Returns the exit code: 0, or 2 when FILE cannot
// be written (perror(prog)).
int write_dry_run(const std::string &path, const char *prog, const std::vector<int32_t> &parent, const ProbeSet &ps,
                  const std::vector<std::string> &labels, const std::vector<SourceOpener> &files, size_t batch_reads, int k);

} // namespace kidhost
