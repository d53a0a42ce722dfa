// kid_side.cpp -- the side options, the side files and what writes them: one table row per option, per file and per
// tallied sample
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>

#include "kid_driver.h"

namespace kidhost {

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
static void read_segment_votes(SideOptions &o, const char *prog, const char *opt, const char *v) { o.segment_votes = parse_segments(prog, opt, v); }

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

static void read_fragment_loci(SideOptions &o, const char *prog, const char *opt, const char *v)
{
    const char *const what = "takes W[:MAX_SPAN], digits only: W in 1..2147483647, MAX_SPAN in 0..2147483647";
    unsigned long long w = 0, span = 1000;
    size_t at = 0;
    if (digits_up_to(0x7FFFFFFFull, v, at, w) <= 0) usage_error(prog, opt, what); // (an empty part too)
    if (v[at] == ':' && digits_up_to(0x7FFFFFFFull, v, ++at, span) <= 0) usage_error(prog, opt, what);
    if (v[at] != 0 || w < 1) usage_error(prog, opt, what); // (a third part too)
    o.fragment_loci = true;
    o.fragment_loci_bin = (uint32_t)w;
    o.fragment_loci_span = (uint32_t)span;
}

// The side options: their words and what reads the value of each -- or, for a switch, which takes none, the flag it sets
// -- and whether it is an option of nk10 alone (such an option names the flag that says it is on, a valued one too).  The rows stand in the order in which malformed values are diagnosed; an
// option whose row has new_group set is diagnosed behind every option of the rows above it, the options of one group in
// their order on the command line.  (A switch cannot be malformed: the switches stand where they disturb no group.)
static const struct {
    const char *name;
    bool new_group;
    void (*read)(SideOptions &, const char *prog, const char *opt, const char *v);
    bool SideOptions::*flag;
    bool nk10_alone;
} kSideOptions[] = {{"--min-hits", true, read_min_hits, nullptr, false},
                    {"--confidence", false, read_confidence, nullptr, false},
                    {"--hits", false, nullptr, &SideOptions::hits, false},
                    {"--depth", false, nullptr, &SideOptions::depth, false},
                    {"--seen", false, nullptr, &SideOptions::seen, false},
                    {"--fragments", false, nullptr, &SideOptions::fragments, true},
                    {"--votes", false, nullptr, &SideOptions::votes, false},
                    {"--fragment-votes", false, nullptr, &SideOptions::fragment_votes, true},
                    {"--min-base-quality", true, read_base_quality, nullptr, false},
                    {"--low-complexity", false, read_low_complexity, nullptr, false},
                    {"--segments", true, read_segments, nullptr, false},
                    {"--segment-votes", true, read_segment_votes, nullptr, false},
                    {"--loci", true, read_loci, nullptr, false},
                    {"--pileup", true, read_pileup, nullptr, false},
                    {"--fragment-loci", true, read_fragment_loci, &SideOptions::fragment_loci, true}};

int side_option_values(const char *word)
{
    for (const auto &so : kSideOptions)
        if (strcmp(word, so.name) == 0) return so.read ? 1 : 0;
    return -1;
}

SideOptions side_options(int argc, char **argv, const char *prog)
{
    SideOptions o;
    const size_t n = sizeof(kSideOptions) / sizeof(kSideOptions[0]);
    // one pass over the words per group of rows
    for (size_t lo = 0, hi; lo < n; lo = hi) {
        for (hi = lo + 1; hi < n && !kSideOptions[hi].new_group; hi++) {}
        for (int i = 1; i < argc; i++)
            for (size_t s = lo; s < hi; s++) {
                const auto &so = kSideOptions[s];
                if (strcmp(argv[i], so.name) != 0) continue;
                if (!so.read) { o.*so.flag = true; continue; }
                if (i + 1 >= argc) usage_error(prog, so.name, "needs a value");
                so.read(o, prog, so.name, argv[i + 1]);
            }
    }
    return o;
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
    for (const auto &so : kSideOptions)
        if (so.nk10_alone && o.side.*so.flag)
            usage_error(argv[0], so.name, "is an option of nk10 alone: the inputs of this program are read one file after the other");
    return o;
}

const TallyRow kTallies[TALLY_COUNT] = {
    // a second sample that the support pass tallies every batch into under the rule (kid_db_read_support*:
    // gcount[confident]++ where the result file has gcount[final]++); --depth switches its depth counters on
    {[](const SideOptions &o) { return o.support.on || o.depth; }, true},
    // every fragment is tallied into it (kid_db_read_fragments_fastq), dealt over the devices
    {[](const SideOptions &o) { return o.fragments; }, false},
    // the vote pass tallies every batch into it (kid_db_read_votes*)
    {[](const SideOptions &o) { return o.votes; }, false},
    // the fragments called by votes (kid_db_read_fragment_votes_fastq), dealt with the fragments
    {[](const SideOptions &o) { return o.fragment_votes; }, false}};

// What fills a side file: the counters of a tallied sample, the lines that the batches left with SampleOutputs::add, or a
// writer of its own
enum Fill { FILL_TALLY, FILL_LINES, FILL_DEPTH, FILL_SEEN, FILL_PILEUP };

// The side files, in the order of SideFile: the file stands beside the result file under its path with the last
// `replaces` replaced by `word` (".../x_result.txt" -> ".../x_hits.txt"; a path without one gets `or_appends` behind
// it); it is on -- removed when a sample starts, written when it is finished -- under the options `on` says.
// Wherever a rule is named it is that of --min-hits / --confidence when given, else (0, 0); --min-base-quality and
// --low-complexity apply to every file; none depends on how the reads were cut into blocks, batched, threaded or dealt
// over devices.
static const struct {
    const char *replaces, *word, *or_appends;
    bool (*on)(const SideOptions &);
    Fill fill;
    Tally tally; // the tallied sample whose counters, depth spectrum or seen-bitmap it holds
} kSideFiles[SF_COUNT] = {
    // --min-hits / --confidence: a result file in the result file's format, of the reads the rule calls.  (Not on under
    // --depth alone, which has the sample tallied without a rule.)
    {"result", "confident", "", [](const SideOptions &o) { return o.support.on; }, FILL_TALLY, TALLY_CONFIDENT},
    // --fragments (nk10): a result file in the result file's format, <i>,<fragments>,<unique_kmers>.  Record j of the R1
    // file and record j of the R2 file are one fragment, j counting the 4-line records of each file, those that
    // process_qual drops included; header names are not compared.  The surplus records of the longer file (all of them
    // when R2 is missing) are fragments with an absent mate, and one line on stderr gives both counts.  Under the rule.
    {"result", "fragments", "", [](const SideOptions &o) { return o.fragments; }, FILL_TALLY, TALLY_FRAGMENTS},
    // --votes: a result file in the result file's format, <i>,<reads>,<unique_kmers>: gcount[confident]++ with the climb
    // started at the read's call by root-path votes, which does not depend on the order of its hits.  Under the rule:
    // without one confident = call.  The depth and seen files keep following the samples they follow without it.
    {"result", "votes", "", [](const SideOptions &o) { return o.votes; }, FILL_TALLY, TALLY_VOTES},
    // --fragment-votes (nk10): a result file in the result file's format, <i>,<fragments>,<unique_kmers>: the fragments of
    // --fragments (the same pairing of records, the same blocks, absent mates and stderr line -- printed once when both
    // options are given), each called by root-path votes over the hits of both mates, which does not depend on the order
    // of the mates or of their hits.  Under the rule.  It needs neither --fragments nor --votes and changes nothing they write.
    {"result", "fragment_votes", "", [](const SideOptions &o) { return o.fragment_votes; }, FILL_TALLY, TALLY_FRAGMENT_VOTES},
    // --depth: ntar lines <i>,<kmer_hits>,<distinct>,<q1>,<q2>,<q3>,<max>, integers, from the depth spectrum (256 bins) of
    // the confident sample(s): the hits on the target's database k-mers by the reads the rule calls, how many of its
    // k-mers were hit, the quartiles of their depth (the smallest d >= 1 with 4 * #{1 <= depth <= d} >= p * distinct;
    // depths of 255 and more count as 255; 0 without a hit) and the largest depth.  Its column 3 is the column 3 of the
    // confident file, or of the result file without a rule.
    {"result", "depth", "", [](const SideOptions &o) { return o.depth; }, FILL_DEPTH, TALLY_CONFIDENT},
    // --seen: a 32-byte little-endian header (SeenHeader) and the seen-bitmap, one bit per database entry in the layout of
    // kid_sample_seen_export: the union over the devices, of the confident sample(s) under --min-hits / --confidence, else
    // of the classified one(s) -- the convention of the depth file's `distinct` column.
    {"result.txt", "seen.bin", ".seen.bin", [](const SideOptions &o) { return o.seen; }, FILL_SEEN, TALLY_CONFIDENT},
    // --hits: one line per read that was handed to process_read and has at least one k-mer hit, in the reference's read
    // order (all of file 0, then file 1, ...), tab-separated, the header line last:
    //   <final_targ> <trimmed length> <n_kmers> <n_hits> <pos>:<target>:<entry> ... <header line as in _reads.txt>
    {"result", "hits", "", [](const SideOptions &o) { return o.hits; }, FILL_LINES, TALLY_COUNT},
    // --segments LEN[:STEP]: one line per read with a hit, in the order of the hits file, with the segments that have one:
    //   <final_targ> <trimmed length> <n_segments> <segments with a hit> <pos>:<n_pos>:<n_kmers>:<n_hits>:<final>:<confident> ... <header>
    // Under the rule: without one confident = final.
    {"result", "segments", "", [](const SideOptions &o) { return o.segments.on; }, FILL_LINES, TALLY_COUNT},
    // --segment-votes LEN[:STEP]: the lines of the segments file, in its order, for the segments of its own geometry called
    // by root-path votes, which does not depend on the order of a segment's hits.  Under the rule.
    //   <final_targ> <trimmed length> <n_segments> <segments with a hit> <pos>:<n_pos>:<n_kmers>:<n_hits>:<call>:<confident>:<p_best>:<n_best> ... <header>
    {"result", "segment_votes", "", [](const SideOptions &o) { return o.segment_votes.on; }, FILL_LINES, TALLY_COUNT},
    // --loci W: one line per read with a hit, in the order of the hits file (kid_db_read_loci* with diag_bin = W):
    //   <final_targ> <trimmed length> <n_kmers> <n_hits> <org>:<strand>:<n_chain>:<n_org>:<n_other>:<pos_first>:<pos_last>:<pos[entry_first]> <header>
    {"result", "loci", "", [](const SideOptions &o) { return o.loci.on; }, FILL_LINES, TALLY_COUNT},
    // --pileup W[:MIN_CHAIN[:MIN_MARGIN]]: the loci records of every batch (diag_bin = --loci's W when given, else 1) added to
    // the batch's device's pileup of bin width W under (MIN_CHAIN, MIN_MARGIN); at the sample's end the devices' pileups
    // are merged and summed up per organism.  Integers only; n_records the reads that were handed to process_read, and one
    // line for every organism with n_placed >= 1, in ascending order:
    //   #<n_records>,<n_placed>,<W>,<MIN_CHAIN>,<MIN_MARGIN>
    //   <org>,<n_placed>,<span_bins>,<bins_covered>,<max_gap>,<max_depth>,<max_depth_bin>,<max_starts>,<max_starts_bin>,<depth_sum>
    {"result", "pileup", "", [](const SideOptions &o) { return o.pileup.on; }, FILL_PILEUP, TALLY_COUNT},
    // --fragment-loci W[:MAX_SPAN] (nk10): the fragments of --fragments (the same pairing of records, the same blocks, absent
    // mates and stderr line -- printed once whatever combination of the three fragment options is given), each placed by
    // kid_db_read_fragment_loci_fastq with diag_bin = W and max_span = MAX_SPAN.  One line per fragment with n_hits >= 1, in
    // ascending j, the 0-based index of the 4-line record in its files, tab-separated:
    //   <j> <n_kmers> <n_hits> <org>:<orient>:<mates>:<n_chain>:<n_chain_1>:<n_chain_2>:<n_org>:<n_other>:<lo>:<hi>
    {"result", "fragment_loci", "", [](const SideOptions &o) { return o.fragment_loci; }, FILL_LINES, TALLY_COUNT}};

static std::string side_path(const std::string &result_path, int which)
{
    const auto &row = kSideFiles[which];
    std::string p = result_path;
    const size_t at = p.rfind(row.replaces);
    if (at != std::string::npos) p.replace(at, strlen(row.replaces), row.word);
    else p += row.or_appends;
    return p;
}

void remove_side_files(const std::string &result_path, const SideOptions &side, bool all)
{
    for (int f = 0; f < SF_COUNT; f++)
        if (all || kSideFiles[f].on(side)) remove(side_path(result_path, f).c_str());
}

SampleOutputs::SampleOutputs(const std::string &result_path, const SideOptions &side) : side_(side), result_path_(result_path)
{
    remove_side_files(result_path, side);
}

bool SampleOutputs::on(SideFile which) const { return kSideFiles[which].on(side_); }

void SampleOutputs::add(SideFile which, size_t file, const std::string &lines)
{
    std::vector<std::string> &to = lines_[which];
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

// The depth spectrum of a tallied sample (one per device, merged) -> the depth file
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

// The pileups of a sample (one per device: the others are merged into the first; kid_pileup_export, kid_pileup_merge) ->
// the head line and one line per organism with a placed read
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
    write_counters(e.samples, e.ntar, result_path_);
    for (int f = 0; f < SF_COUNT; f++) {
        const auto &row = kSideFiles[f];
        if (!row.on(side_)) continue;
        const std::string path = side_path(result_path_, f);
        switch (row.fill) {
        case FILL_TALLY: write_counters(e.tallied[row.tally], e.ntar, path); break;
        case FILL_LINES: write_lines(path, lines_[f]); break;
        case FILL_DEPTH: write_depth(e.tallied[row.tally], e.ntar, path); break;
        case FILL_SEEN: write_seen(side_.support.on ? e.tallied[row.tally][0] : e.samples[0], e, path); break; // (without a rule: the classified ones')
        case FILL_PILEUP:
            if (!e.pileups.empty()) write_pileup(e.pileups, side_.pileup, path);
            break;
        }
    }
    for (std::vector<std::string> &l : lines_) l.clear();
}

} // namespace kidhost
