// kid_side.h -- the side options the three front-ends (nk10, kmer_read_vf6, kmer_read_m3) share and the files they write
// beside a sample's result file.  kid_side.cpp has one table row per option, per file and per tallied sample: a new side
// output is described there ("adding a side output").
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace kidhost {

struct Engine;

// Each side option gives a sample / job one more output beside its result file (SideFile below) or changes what the GPU
// reads.  All are checked, then ignored, with --dry-run.
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
    // are read as 'N' by everything that runs on the GPU (KID_OPT_MIN_BASE_QUALITY / KID_DB_OPT_MIN_BASE_QUALITY): every
    // side file and stdout are what they would be on input files with those bases replaced by N; the reads file prints
    // the sequences as they are in the input.  FASTQ.gz blocks are masked by the library behind their upload; the batches
    // of a plain FASTQ file carry their qualities (ReadBatch::quals) and are masked through kid_mask_batch before they are
    // classified (run_files).  FASTA input has no qualities: the option is accepted and changes nothing.
    int min_base_quality = 0;
    // --low-complexity T (digits only, 0..1000; 0 = off, the default; 20 is DUST's usual level): the bases that lie in a
    // low-complexity window (kmer_id_amd.h, "mask low-complexity sequence") are read as 'N' in the same way
    // (KID_OPT_LOW_COMPLEXITY / KID_DB_OPT_LOW_COMPLEXITY), behind the quality mask when both are given.  Plain FASTQ and
    // FASTA input go through kid_lowc_batch into the same masked copy: unlike the quality option, this one applies to FASTA.
    int low_complexity = 0;
    SegmentsOption segments;
    // --depth (no value): k-mer depth per database entry (KID_OPT_ENTRY_DEPTH).  The support pass runs for it under the rule
    // of --min-hits / --confidence when given, else (0, 0).
    bool depth = false;
    bool seen = false;           // --seen (no value): the sample's seen-bitmap, for kmer_shared to compare samples by
    bool fragments = false;      // --fragments (no value; nk10 alone, whose two mate files are read side by side)
    bool votes = false;          // --votes (no value): the reads called by root-path votes
    bool fragment_votes = false; // --fragment-votes (no value; nk10 alone, like --fragments)
    // --segment-votes LEN[:STEP] (the value grammar of --segments).  Independent of --segments: both may be given, with
    // different geometries, and neither changes what the other writes.
    SegmentsOption segment_votes;
    // --loci W.  The probes are loaded with their sites (load_database's want_sites) and every replica of the database gets
    // them (engine_open).
    LociOption loci;
    // --pileup W[:MIN_CHAIN[:MIN_MARGIN]].  It loads the sites as --loci does and runs the loci pass where --loci runs it, with
    // --loci's diagonal bin when that is given, else 1: with both options one loci pass per batch feeds both files.
    PileupOption pileup;
    // --fragment-loci W[:MAX_SPAN] (nk10 alone, like --fragments): place the mate pairs as one fragment by colinear hits
    // (kid_db_read_fragment_loci_fastq).  Digits only; W, the diagonal bin width, in 1..2147483647; MAX_SPAN, the largest
    // (E - D) * W of a paired placement in bases, in 0..2147483647, default 1000.  It loads the sites as --loci does and pairs
    // the records exactly as --fragments does.
    bool fragment_loci = false;
    uint32_t fragment_loci_bin = 0, fragment_loci_span = 1000;
};
// The one place that reads them.  Every word of argv that is an option's name is an occurrence and the word behind it
// its value; a later occurrence overrides an earlier one.  A missing or malformed value (an empty part or a second colon
// of --segments or --segment-votes, a fourth part of --pileup or a third of --fragment-loci too) is a usage error: "<prog>: <option> <what>" on stderr
// and exit code 2 -- of several, the first in the order of the option table's groups (--min-hits / --confidence,
// --min-base-quality / --low-complexity, --segments, --segment-votes, --loci, --pileup, --fragment-loci); within a group, the first in argv.
SideOptions side_options(int argc, char **argv, const char *prog);
// For a front-end that rejects the words it does not know: the number of value words behind `word` (0 or 1) if it
// is a side option, else -1
int side_option_values(const char *word);

// The options kmer_read_vf6 and kmer_read_m3 share, read the way the reference reads its own: a flag takes the next word
// as its value (and that word is looked at as a flag too), a word that is no option is ignored.
struct ReaderOptions {
    int k = 30, log2_slots = 30, device = 0, threads = 0;
    std::string device_list; // --devices: replicas of the table, batches dealt round-robin, counters merged
    size_t batch_reads = 1 << 18;
    std::string dry_run;     // --dry-run FILE: host stages only (no GPU), for the CPU test-suite
    std::string db_cache;    // --db-cache FILE: binary cache of the parsed database
    SideOptions side;        // side_options() of the same words; those of nk10 alone are usage errors
};
ReaderOptions parse_reader_options(int argc, char **argv, int default_threads);

// The files a sample / job may have beside its result file, in the order they are written.  kid_side.cpp has a row for
// each: its name, the options it is on under, what fills it, and its format.
enum SideFile { SF_CONFIDENT, SF_FRAGMENTS, SF_VOTES, SF_FRAGMENT_VOTES, SF_DEPTH, SF_SEEN, SF_HITS, SF_SEGMENTS, SF_SEGMENT_VOTES, SF_LOCI, SF_PILEUP, SF_FRAGMENT_LOCI, SF_COUNT };

// The samples beside the classified one that an engine holds per device, each tallied into by a pass over every batch
// (or fragment) and written as a result file of its own (the row of the side file names its tally)
enum Tally { TALLY_CONFIDENT, TALLY_FRAGMENTS, TALLY_VOTES, TALLY_FRAGMENT_VOTES, TALLY_COUNT };
struct TallyRow {
    bool (*wanted)(const SideOptions &); // the engine has these samples under these options
    // --min-base-quality / --low-complexity are set on these samples as on the classified ones; the others are tallied
    // through the database's hit pass alone, and the database's option is what masks for them
    bool own_masks;
};
extern const TallyRow kTallies[TALLY_COUNT];

// A sample's side files.  Nothing else changes under any of the options: the result and reads files and stdout are what
// they are without.  The batches of files read at the same time interleave: the lines of the files that hold one per
// read are held in memory per input file and written in file order by finish() -- what is held is the files themselves
// (reads without a hit leave nothing), nothing else.  A sample that is not finished (it failed) leaves none of them.
class SampleOutputs {
public:
    // removes the files that are on, left there by an earlier run
    SampleOutputs(const std::string &result_path, const SideOptions &side);
    bool on(SideFile which) const;
    const std::string &result_path() const { return result_path_; }
    // the lines of a batch of input file `file` for a side file that is filled with lines
    void add(SideFile which, size_t file, const std::string &lines);
    // gcount / ucount of the sample -> "<i>,<g>,<u>" lines in the result file, then every side file that is on
    void finish(Engine &e);
private:
    SideOptions side_;
    std::string result_path_;
    std::vector<std::string> lines_[SF_COUNT]; // [input file]
};
// For a front-end that takes a sample's outputs back: removes the files beside `result_path` that are on (a sample that
// never started: one left by an earlier run would stand beside no result) or, with `all`, every one a sample may have written
void remove_side_files(const std::string &result_path, const SideOptions &side, bool all = false);

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

} // namespace kidhost
