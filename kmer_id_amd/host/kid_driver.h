// kid_driver.h -- what the three front-ends (nk10, kmer_read_vf6, kmer_read_m3) share: the database
// on the GPU, the reader-thread / GPU-thread pipeline over the input files, closing a sample.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "kid_host.h"
#include "kmer_id_amd.h"

namespace kidhost {

// The side options the three front-ends share: each gives a sample / job one more output beside its result file
// (SampleOutputs below has the files) or changes what the GPU reads.  All are checked, then ignored, with --dry-run.
// --min-hits N / --confidence F: call reads by k-mer support.  Either option switches the feature on, the one not given
// is 0.  N: a decimal number up to 2^32-1.  F: a decimal in [0, 1] with at most three fractional digits, turned into
// permille from its digits.
struct SupportRule {
    bool on = false;
    uint32_t min_hits = 0, min_permille = 0;
};
// --segments LEN[:STEP]: call long records in segments (kid_db_read_segments*).  Digits only; LEN in 1..2147483647 window
// positions; STEP (default LEN) in 1..LEN with LEN <= 1024 * STEP.
struct SegmentsOption {
    bool on = false;
    uint32_t seg_len = 0, seg_step = 0;
};
// --loci W: place reads on a genome by colinear hits (kid_db_read_loci*).  Digits only; W, the diagonal bin width, in
// 1..2147483647.
struct LociOption {
    bool on = false;
    uint32_t diag_bin = 0;
};
// --pileup W[:MIN_CHAIN[:MIN_MARGIN]]: pile the placed reads up per genome bin (kid_pileup_*).  Digits only; W, the bin
// width, in 1..2147483647; MIN_CHAIN in 1..4096, default 2; MIN_MARGIN in 0..4096, default 1.
struct PileupOption {
    bool on = false;
    uint32_t bin_width = 0, min_chain = 2, min_margin = 1;
};
struct SideOptions {
    bool hits = false;   // --hits: every read's k-mer hits
    SupportRule support;
    // --min-base-quality Q (digits only, 0..93; 0 = off, the default): the bases of FASTQ input whose quality is below Q
    // are read as 'N' by everything that runs on the GPU (KID_OPT_MIN_BASE_QUALITY / KID_DB_OPT_MIN_BASE_QUALITY): the
    // result, hits and confident files and stdout are what they would be on input files with those bases replaced by N;
    // the reads file prints the sequences as they are in the input.  FASTQ.gz blocks are masked by the library behind
    // their upload; the batches of a plain FASTQ file carry their qualities (ReadBatch::quals) and are masked through
    // kid_mask_batch before they are classified (run_files).  FASTA input has no qualities: the option is accepted and
    // changes nothing.
    int min_base_quality = 0;
    // --low-complexity T (digits only, 0..1000; 0 = off, the default; 20 is DUST's usual level): the bases that lie in a
    // low-complexity window (kmer_id_amd.h, "mask low-complexity sequence") are read as 'N' in the same way
    // (KID_OPT_LOW_COMPLEXITY / KID_DB_OPT_LOW_COMPLEXITY), behind the quality mask when both are given.  Plain FASTQ and
    // FASTA input go through kid_lowc_batch into the same masked copy: unlike the quality option, this one applies to FASTA.
    int low_complexity = 0;
    SegmentsOption segments;
    // --depth (no value): k-mer depth per database entry (KID_OPT_ENTRY_DEPTH), summed up per target in a depth file.  The
    // support pass runs for it under the rule of --min-hits / --confidence when given, else (0, 0).
    bool depth = false;
    // --seen (no value): the sample's seen-bitmap in a seen file, for kmer_shared to compare samples by
    bool seen = false;
    // --fragments (no value; nk10 alone, whose two mate files are read side by side): the mate pairs called as one
    // fragment each (kid_db_read_fragments_fastq), counted into a fragments file
    bool fragments = false;
    // --votes (no value): the reads called by root-path votes (kid_db_read_votes*), whatever the order of their hits, and
    // counted into a votes file
    bool votes = false;
    // --fragment-votes (no value; nk10 alone, like --fragments): the mate pairs called by root-path votes over both mates'
    // hits (kid_db_read_fragment_votes_fastq), counted into a fragment_votes file
    bool fragment_votes = false;
    // --segment-votes LEN[:STEP] (the value grammar of --segments): long records called in segments by root-path votes
    // (kid_db_read_segment_votes*), into a segment_votes file.  Independent of --segments: both may be given, with
    // different geometries, and neither changes what the other writes.
    SegmentsOption segment_votes;
    // --loci W: every read with a hit placed on a genome by its colinear hits, into a loci file.  The probes are loaded
    // with their sites (load_database's want_sites) and every replica of the database gets them (engine_open).
    LociOption loci;
    // --pileup W[:MIN_CHAIN[:MIN_MARGIN]]: the loci records of every batch piled up per genome bin of W bases, summed up per
    // organism in a pileup file.  It loads the sites as --loci does and runs the loci pass where --loci runs it, with
    // --loci's diagonal bin when that is given, else 1: with both options one loci pass per batch feeds both files.
    PileupOption pileup;
};
// The one place that reads them.  Every word of argv that is an option's name is an occurrence and the word behind it
// its value; a later occurrence overrides an earlier one.  A missing or malformed value (an empty part or a second colon
// of --segments or --segment-votes, a fourth part of --pileup too) is a usage error: "<prog>: <option> <what>" on stderr and exit code 2 -- of several, the first in
// the order --min-hits / --confidence, --min-base-quality / --low-complexity, --segments, --segment-votes, --loci, --pileup.
SideOptions side_options(int argc, char **argv, const char *prog);
// For a front-end that rejects the words it does not know: the number of value words behind `word` (0 or 1) if it
// is a side option, else -1
int side_option_values(const char *word);

struct Engine {
    kid_db *db = nullptr;         // the database on the first device
    kid_sample *sample = nullptr; // ... and its sample
    // one replica of the database + one sample per device (--devices a,b,...): [0] are the two above.  The batches of
    // a file are dealt round-robin over the samples, the per-read results come back in file order, and closing a
    // sample merges the replicas' counters (kid_sample_end_merged).
    std::vector<kid_db *> dbs;
    std::vector<kid_sample *> samples;
    size_t next_sample = 0;
    // the side options (engine_configure) and, under --min-hits / --confidence or --depth, one tallied sample per device
    // (with the depth counters on under --depth)
    SideOptions side;
    std::vector<kid_sample *> confident;
    std::vector<kid_sample *> fragments; // under --fragments: one sample per device that the fragments are tallied into
    size_t next_fragments = 0;           // ... dealt round-robin over the devices
    std::vector<kid_sample *> votes;     // under --votes: one sample per device that the vote pass of every batch tallies into
    std::vector<kid_sample *> fragment_votes; // under --fragment-votes: one per device for the fragments called by votes (dealt with `fragments`)
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
// The side options for an engine that is open: with a rule or --depth one more sample per device (reset, closed and
// destroyed with the others; --depth switches its depth counters on), under --fragments one more for the fragments, under
// --votes one more for the vote pass, under --fragment-votes one more for the fragments called by votes, under --pileup one pileup per device (the sites are there: engine_open), then --min-base-quality and --low-complexity on every sample, the tallied ones included, and on every replica of the database.
// A worker of engine_worker() inherits them for its samples.
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

// The files a sample / job has beside its result file, each named like it with the last "result" replaced by a word
// (".../x_result.txt" -> ".../x_hits.txt"), and when they are removed and written.
//   --hits, "hits": one line per read that was handed to process_read and has at least one k-mer hit, in the
// reference's read order (all of file 0, then file 1, ...), tab-separated, the header line last:
//   <final_targ> <trimmed length> <n_kmers> <n_hits> <pos>:<target>:<entry> ... <header line as in _reads.txt>
//   --min-hits / --confidence, "confident": a result file in the result file's format, from the counters of a second
// sample per device that is tallied with every batch under the rule (kid_db_read_support*: gcount[confident]++ where
// the result file has gcount[final]++).
//   --segments, "segments": one line per read that was handed to process_read and has at least one k-mer hit, in the
// order of the hits file, tab-separated, the header line last:
//   <final_targ> <trimmed length> <n_segments> <segments with a hit> <pos>:<n_pos>:<n_kmers>:<n_hits>:<final>:<confident> ... <header>
//   --depth, "depth": ntar lines <i>,<kmer_hits>,<distinct>,<q1>,<q2>,<q3>,<max>, integers, from the depth spectrum
// (256 bins) of the tallied sample(s): the hits on the target's database k-mers by the reads the rule calls, how many of
// its k-mers were hit, the quartiles of their depth (the smallest d >= 1 with 4 * #{1 <= depth <= d} >= p * distinct;
// depths of 255 and more count as 255; 0 without a hit) and the largest depth.  Its column 3 is the column 3 of the
// confident file, or of the result file without a rule.
//   --seen, "seen": the final "result.txt" of the name becomes "seen.bin".  A 32-byte little-endian header (SeenHeader) and
// the seen-bitmap, one bit per database entry in the layout of kid_sample_seen_export: the union over the devices, of the
// tallied sample(s) under a rule (--min-hits / --confidence), else of the classified one(s) -- the convention of the depth
// file's `distinct` column, so its bits per target are column 3 of the confident file under a rule, of the result file
// without.  It does not depend on how the reads were batched, threaded or dealt over devices.
// Only the segments with a hit are listed.  The rule is that of --min-hits / --confidence when given, else (0, 0):
// confident = final.  --min-base-quality applies as it does to the hits file.
//   --fragments, "fragments" (nk10): a result file in the result file's format, <i>,<fragments>,<unique_kmers>, from the
// counters of one more sample per device that every fragment is tallied into (kid_db_read_fragments_fastq): record j
// of the R1 file and record j of the R2 file are one fragment, j counting the 4-line records of each file, those that
// process_qual drops included; header names are not compared.  The surplus records of the longer file (all of them
// when R2 is missing) are fragments with an absent mate, and one line on stderr gives both counts.  The rule is that of
// --min-hits / --confidence when given, else (0, 0); --min-base-quality applies as it does to the confident file.  It
// does not depend on how the files were cut into blocks, batched, threaded or dealt over devices.
//   --votes, "votes": a result file in the result file's format, <i>,<reads>,<unique_kmers>, from the counters of one more
// sample per device that the vote pass tallies every batch into (kid_db_read_votes*: gcount[confident]++ with the climb
// started at the read's call by root-path votes, which does not depend on the order of its hits).  The rule is that of
// --min-hits / --confidence when given, else (0, 0): confident = call; --min-base-quality applies as it does to the
// confident file.  It does not depend on how the reads were batched, threaded or dealt over devices, and the depth and
// seen files keep following the samples they follow without it.
//   --fragment-votes, "fragment_votes" (nk10): a result file in the result file's format, <i>,<fragments>,<unique_kmers>,
// from the counters of one more sample per device that every fragment is tallied into by
// kid_db_read_fragment_votes_fastq: the fragments of --fragments (the same pairing of records, the same blocks, absent
// mates and stderr line -- printed once when both options are given), each called by root-path votes over the hits of both
// mates, which does not depend on the order of the mates or of their hits.  The rule is that of --min-hits / --confidence
// when given, else (0, 0); --min-base-quality and --low-complexity apply as they do to the fragments file.  It needs
// neither --fragments nor --votes, changes nothing they write, and does not depend on how the files were cut into
// blocks, batched, threaded or dealt over devices.
//   --segment-votes, "segment_votes": the lines of the segments file, in its order, for the segments of its own LEN[:STEP]
// called by root-path votes (kid_db_read_segment_votes*), which does not depend on the order of a segment's hits:
//   <final_targ> <trimmed length> <n_segments> <segments with a hit> <pos>:<n_pos>:<n_kmers>:<n_hits>:<call>:<confident>:<p_best>:<n_best> ... <header>
// Only the segments with a hit are listed.  The rule is that of --min-hits / --confidence when given, else (0, 0);
// --min-base-quality and --low-complexity apply as they do to the segments file.  It does not depend on how the reads
// were batched, threaded or dealt over devices, and needs --segments no more than --segments needs it.
//   --loci W, "loci": one line per read that was handed to process_read and has at least one k-mer hit, in the order of
// the hits file, tab-separated, the header line last (kid_db_read_loci* with diag_bin = W on the batch's device):
//   <final_targ> <trimmed length> <n_kmers> <n_hits> <org>:<strand>:<n_chain>:<n_org>:<n_other>:<pos_first>:<pos_last>:<pos[entry_first]> <header>
// --min-base-quality and --low-complexity apply as they do to the hits file.  It does not depend on how the reads were
// batched, threaded or dealt over devices.
//   --pileup W[:MIN_CHAIN[:MIN_MARGIN]], "pileup": the loci records of every batch (diag_bin = --loci's W when given, else 1)
// added to the batch's device's pileup of bin width W under (MIN_CHAIN, MIN_MARGIN); at the sample's end the devices'
// pileups are merged (kid_pileup_export, kid_pileup_merge) and summed up per organism.  Integers only:
//   #<n_records>,<n_placed>,<W>,<MIN_CHAIN>,<MIN_MARGIN>
//   <org>,<n_placed>,<span_bins>,<bins_covered>,<max_gap>,<max_depth>,<max_depth_bin>,<max_starts>,<max_starts_bin>,<depth_sum>
// n_records the reads that were handed to process_read, and one line for every organism with n_placed >= 1, in ascending order.  --min-base-quality and --low-complexity apply as they
// do to the loci file.  It does not depend on how the reads were batched, threaded or dealt over devices.
// Nothing else changes under any of them: the result and reads files and stdout are what they are without.
// The batches of files read at the same time interleave: the hit, segment, segment_votes and loci lines are held in memory per file and
// written in file order by finish() -- what is held is the files themselves (reads without a hit leave nothing),
// nothing else.  One that is not finished (its sample failed) leaves no hits, no segments, no segment_votes and no loci file.
class SampleOutputs {
public:
    // removes the files of the options that are on, left there by an earlier run
    SampleOutputs(const std::string &result_path, const SideOptions &side);
    bool hits_on() const { return side_.hits; }
    bool segments_on() const { return side_.segments.on; }
    bool fragments_on() const { return side_.fragments; }
    bool fragment_votes_on() const { return side_.fragment_votes; }
    bool segment_votes_on() const { return side_.segment_votes.on; }
    bool loci_on() const { return side_.loci.on; }
    bool pileup_on() const { return side_.pileup.on; }
    const std::string &result_path() const { return result_path_; }
    void add_hits(size_t file, const std::string &lines) { add(hits_, file, lines); }
    void add_segments(size_t file, const std::string &lines) { add(segments_, file, lines); }
    void add_segment_votes(size_t file, const std::string &lines) { add(segment_votes_, file, lines); }
    void add_loci(size_t file, const std::string &lines) { add(loci_, file, lines); }
    // gcount / ucount of the sample -> "<i>,<g>,<u>" lines in the result file, those of the tallied sample(s) -> the
    // confident file, then the fragments file, then the votes file, then the fragment_votes file, then the depth file, then the seen file, then the hits file, then the
    // segments file, then the segment_votes file, then the loci file, then the pileup file
    void finish(Engine &e);
private:
    using Lines = std::vector<std::string>; // [file]
    static void add(Lines &to, size_t file, const std::string &lines);
    SideOptions side_;
    std::string result_path_;
    Lines hits_, segments_, segment_votes_, loci_;
};
// The head of a seen file: the 8 bytes "KIDSEEN1", then these fields, little-endian, 32 bytes in all; nbytes bytes of
// bitmap follow (the padded size of a database of n_entries: ((n_entries + 127) / 128) * 16, 16 for none)
struct SeenHeader {
    uint64_t n_entries = 0;
    int32_t ntar = 0, k = 0;
    uint64_t nbytes = 0;
};
extern const char kSeenMagic[9];
// The seen files of a tool that compares them (kmer_shared, kmer_coverage), in the order of `paths`: maps[f] receives the
// bitmap of file f, `first` the header of the first file.  Every header must fit its file, agree with the first file's
// (entries, targets, k) and with the tool's own k and, unless ntar is negative, ntar.  Returns 0, or the exit code of the
// first file that fails -- 255 for one that cannot be opened, 3 for a bad magic, a truncated file, a bitmap whose size
// does not fit its entries, headers that disagree -- with the line for stderr, without the tool's name, in `what`.
int read_seen_files(const std::vector<std::string> &paths, long long ntar, unsigned long long k, std::vector<std::vector<uint8_t>> &maps,
                    SeenHeader &first, std::string &what);
// For a front-end that takes a sample's outputs back: removes the files beside `result_path` of the options that are on
// (a sample that never started: one left by an earlier run would stand beside no result) or, with `all`, every one a
// sample may have written
void remove_side_files(const std::string &result_path, const SideOptions &side, bool all = false);

// Classify the files [first, first + count) of ONE sample, read at the same time (the two mates of nk10: two inflate
// threads instead of one after the other); the counters do not care about the order, the read saver restores it.
// `saver_file` is the saver's index of file `first` (a saver may span several calls: the files of a kmer_read_vf6 job,
// -f1 and -f2 of kmer_read_m3).  done(f, handed), if given, is called for every file first + f in file order once all of
// them are through, with the number of its reads handed to process_read.  Returns the reads handed of all the files.
// `out` receives the hit lines of every batch when its hits file is on: the hit pass (kid_db_read_hits*) of a batch runs on
// the device that classified it, once its final targets are back.  With e.side.support or e.side.depth on, the support
// pass of a batch runs at the same place and tallies into that device's confident sample; with e.side.votes on the vote
// pass (kid_db_read_votes*) does the same into that device's votes sample.  When its segments file is on, `out` receives
// the segment lines of every batch under e.side: the segments pass (kid_db_read_segments*) runs at the same place too,
// and so does the segment-votes pass (kid_db_read_segment_votes*) when its segment_votes file is on.
// With out.fragments_on() or out.fragment_votes_on() and count == 2 the two files are the mates of a sample: the FASTQ blocks of each that are
// through wait in a queue until the partner's records have arrived; the longest common run of records is handed to
// kid_db_read_fragments_fastq with a device's fragment sample as its tally (and, or, to kid_db_read_fragment_votes_fastq
// with that device's fragment_votes sample: the same run of the same blocks), and a block goes as soon as its last
// record has: none is held longer than the other file lags.
long long run_files(Engine &e, Prefetcher &pf, size_t first, size_t count, ReadSaver &saver, SampleOutputs &out, size_t saver_file = 0,
                    const std::function<void(size_t, long long)> &done = nullptr);

// One opener per path, each by `open`, which sets its bool when the file is a plain FASTA that is not there (the
// reference's "nark <name>"): missing[f] holds it for file f once that file is through.  `missing` must not move
// while the files are read.
std::vector<SourceOpener> make_openers(const std::vector<std::string> &paths, int k, std::vector<char> &missing,
                                       std::unique_ptr<ReadSource> (*open)(const std::string &, int, bool *) = open_by_suffix);

// The options kmer_read_vf6 and kmer_read_m3 share, read the way the reference reads its own: a flag takes the next word
// as its value (and that word is looked at as a flag too), a word that is no option is ignored.
struct ReaderOptions {
    int k = 30, log2_slots = 30, device = 0, threads = 0;
    std::string device_list; // --devices: replicas of the table, batches dealt round-robin, counters merged
    size_t batch_reads = 1 << 18;
    std::string dry_run;     // --dry-run FILE: host stages only (no GPU), for the CPU test-suite
    std::string db_cache;    // --db-cache FILE: binary cache of the parsed database
    SideOptions side;        // side_options() of the same words
};
ReaderOptions parse_reader_options(int argc, char **argv, int default_threads);

// --dry-run FILE (host stages only, no GPU): the database and the reads of `files` as they WOULD be handed to the GPU, as
// text, each file under its label (a file without a reader is left out).  Returns the exit code: 0, or 2 when FILE cannot
// be written (perror(prog)).
int write_dry_run(const std::string &path, const char *prog, const std::vector<int32_t> &parent, const ProbeSet &ps,
                  const std::vector<std::string> &labels, const std::vector<SourceOpener> &files, size_t batch_reads, int k);

} // namespace kidhost
