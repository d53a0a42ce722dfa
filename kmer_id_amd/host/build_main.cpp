// kmer_build_vf6 -- command-line compatible replacement of the reference's probe-database builder
// (kmer_build_vf6.cpp, main at :648-848):
//     kmer_build_vf6 -name N -fadir DIR
// reads ./N/N_filter.txt (outgroup accessions, optional), ./N/N_data.txt ("target accession" per line) and
// ./N/N_tree.txt ("parent child" per line), builds the k-mer table from the ingroup genomes on the GPU (phase 1), spoils
// the k-mers of the outgroups (phase 2), and writes ./N/N_probes.txt and ./N/N_count.txt (phase 3).  Stdout, the files
// and the exit status are the reference's, byte for byte, for the same inputs and table size.
// Extra options: --log2-cells L (35) --max-probes N (100000) --genbank-dir DIR (the reference's hard-coded outdir)
// --device D (0) --batch-bases N (2^24) --timing (phase times as one JSON line on stderr)
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <chrono>
#include <fstream>
#include <future>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kid_driver.h"
#include "kid_textio.h"
#include "kmer_id_amd.h"

using namespace kidhost;

namespace {

const int K = 30;

bool file_exists(const std::string &path)
{
    struct stat st;
    return stat(path.c_str(), &st) == 0;
}

// acgt/ACGT -> upper case, anything else -> N (process_fa, :218-261)
struct CleanTable {
    char t[256];
    CleanTable()
    {
        memset(t, 'N', sizeof(t));
        for (const char *p = "ACGT"; *p; ++p) t[(unsigned char)*p] = *p, t[(unsigned char)(*p + 32)] = *p;
    }
} g_clean;

void append_line(std::string &seq, const char *p, size_t n)
{
    if (n == 0) return;
    if (p[0] == '>') {
        seq.push_back('N'); // contig separator
        return;
    }
    const size_t at = seq.size();
    seq.resize(at + n);
    for (size_t i = 0; i < n; ++i) seq[at + i] = g_clean.t[(unsigned char)p[i]];
}

// process_gz (:305-351): '\r' dropped at line end, the unterminated last line dropped, a line of 16 KiB or more fatal
// (GzLineBlocks enforces the last two)
std::string read_gz(const std::string &path)
{
    std::string seq;
    GzLineBlocks in(path);
    TextBlock blk;
    while (in.next(blk)) {
        const char *p = blk.data(), *end = p + blk.len;
        while (p < end) {
            const char *eol = (const char *)memchr(p, '\n', (size_t)(end - p));
            if (!eol) eol = end;
            size_t n = (size_t)(eol - p);
            if (n >= 0x4000) throw Fatal{255, "Buffer to small for input line lengths"}; // the reader checks only lines across blocks
            if (n && p[n - 1] == '\r') --n;
            append_line(seq, p, n);
            p = eol + 1;
        }
    }
    in.close();
    return seq;
}

// load_data2 (:263-295): every whitespace character removed, lines of length <= 1 skipped
std::string read_contigs(const std::string &path, std::string &message)
{
    std::string seq, line;
    std::ifstream fin(path);
    if (!fin.is_open()) {
        message = "could not find " + path + "\n"; // printed by the consumer, in order
        return seq;
    }
    while (std::getline(fin, line)) {
        std::string s;
        s.reserve(line.size());
        for (char c : line)
            if (!(c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r')) s.push_back(c);
        if (s.size() > 1) append_line(seq, s.data(), s.size());
    }
    return seq;
}

// one genome file to read: the candidates in the reference's search order (the first that exists is read)
struct Job {
    std::vector<std::pair<std::string, bool>> paths; // (path, is .gz)
};
struct Loaded {
    int status = 0;     // 0 read, 1 no file, else a Fatal's exit code
    std::string text;
    std::string message;
    std::string could_not_find; // load_data2's message for an unreadable _contigs.fasta (printed in order)
    double seconds = 0;
};

Loaded load(const Job &job)
{
    Loaded r;
    const auto t0 = std::chrono::steady_clock::now();
    r.status = 1;
    for (const auto &pc : job.paths) {
        if (!file_exists(pc.first)) continue;
        try {
            if (pc.second) {
                r.text = read_gz(pc.first);
            } else {
                r.text = read_contigs(pc.first, r.could_not_find);
            }
            r.status = 0;
        } catch (const Fatal &f) {
            r.status = f.exit_code;
            r.message = f.message;
        }
        break;
    }
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return r;
}

std::string kmer_text(uint64_t key)
{
    std::string s(K, 'A');
    for (int i = K - 1; i >= 0; --i, key >>= 2) s[i] = "ACGT"[key & 3];
    return s;
}

int minct_of(int n)
{
    if (n == 1) return 1;
    if (n < 4) return 2;
    if (n < 10) return n - 2;
    return n / 5 + 1;
}

void check(int rc, const char *what)
{
    if (rc != 0) {
        std::cout.flush();
        std::cerr << "kmer_build_vf6: " << what << ": " << kid_strerror(rc) << " (" << kid_last_error() << ")\n";
        leave_now(3); // (a genome reader may still be running: nothing is unwound under it)
    }
}

} // namespace

int main(int argc, char **argv)
{
    std::string name = "bob", wdir, fdir, outdir = "/mnt/dmb/Mark_backup/genbank/";
    int log2_cells = 35, device = 0;
    long max_probes = 100000;
    uint64_t batch_bases = 0;
    bool timing = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : "";
        if (a == "-name") { name = v; wdir = "./" + name + "/"; }
        if (a == "-fadir") fdir = v;
        if (a == "--log2-cells") log2_cells = atoi(v);
        if (a == "--max-probes") max_probes = atol(v);
        if (a == "--genbank-dir") outdir = v;
        if (a == "--device") device = atoi(v);
        if (a == "--batch-bases") batch_bases = (uint64_t)atoll(v);
        if (a == "--timing") timing = true;
    }
    const auto wall0 = std::chrono::steady_clock::now();
    const std::string iname = wdir + name + "_data.txt", tname = wdir + name + "_tree.txt", iname2 = wdir + name + "_filter.txt",
                      oname = wdir + name + "_probes.txt";
    std::ofstream out(oname.c_str()); // truncated here, before anything can fail

    std::vector<std::string> accession, accession2;
    std::vector<int> targno;
    std::string line, acc;
    {
        std::ifstream fin(iname2);
        while (fin && std::getline(fin, line)) {
            std::stringstream ls(line);
            ls >> acc; // a line without a word keeps the accession before (the reference's stream extraction)
            accession2.push_back(acc);
        }
    }
    std::cout << accession2.size() << " outs loaded" << std::endl;
    int num_targ = 0, targi = 0;
    {
        std::ifstream fin(iname);
        while (fin && std::getline(fin, line)) {
            std::stringstream ls(line);
            ls >> targi >> acc;
            accession.push_back(acc);
            targno.push_back(targi);
            if (targi > num_targ) num_targ = targi;
        }
    }
    num_targ++;
    const int num_orgs = (int)accession.size();
    std::cout << num_orgs << " sequences loaded" << std::endl;
    if (num_targ > (1 << 21)) {
        std::cout.flush();
        std::cerr << "kmer_build_vf6: target " << num_targ - 1 << " >= 2^21 does not fit a table cell (target << 11)\n";
        return 2;
    }
    // ntargorgs: counted before the tree is loaded, so every org counts for its own target only (:721-732)
    std::vector<int> ntargorgs(num_targ, 0), minct(num_targ, 0);
    std::vector<long> pcount(num_targ, 0);
    for (int t : targno)
        if (t > 1) ntargorgs[t]++;
    std::vector<int32_t> parent(num_targ < 2 ? 2 : num_targ, 1);
    {
        std::ifstream fin(tname);
        int x = 0, y = 0;
        while (fin && std::getline(fin, line)) {
            std::stringstream ls(line);
            ls >> x >> y;
            if (x >= 0 && y >= 0 && x < num_targ && y < num_targ) parent[y] = x; // Tree1::add_edge (:92-97)
        }
    }
    std::cout << "tree loaded" << std::endl;
    for (int t = 0; t < num_targ; t++) minct[t] = minct_of(ntargorgs[t]);
    minct.resize(parent.size(), 2);

    kid_builder *b = nullptr;
    check(kid_builder_create(device, log2_cells, parent.data(), (int32_t)parent.size(), batch_bases, &b), "kid_builder_create");
    check(kid_builder_set_minct(b, minct.data(), (int32_t)minct.size()), "kid_builder_set_minct");

    // every file in the order the reference reads them; the next one is read while the GPU works on the current one
    struct Step {
        int phase, index;
        Job job;
    };
    std::vector<Step> steps;
    for (int i = 0; i < num_orgs; i++)
        if (targno[i] > 1)
            steps.push_back({1, i, Job{{{fdir + accession[i] + ".fasta.gz", true}, {outdir + accession[i] + ".fasta.gz", true},
                                        {fdir + accession[i] + "_contigs.fasta", false}}}});
    for (int i = 0; i < (int)accession2.size(); i++)
        steps.push_back({2, i, Job{{{outdir + accession2[i] + ".fasta.gz", true}, {fdir + accession2[i] + ".fasta.gz", true}}}});
    for (int i = 0; i < num_orgs; i++)
        if (targno[i] > 1)
            steps.push_back({3, i, Job{{{fdir + accession[i] + ".fasta.gz", true}, {outdir + accession[i] + ".fna.gz", true},
                                        {fdir + accession[i] + "_contigs.fasta", false}}}});

    double read_seconds = 0;
    long tct = 0;
    uint64_t size = 0;
    std::vector<kid_build_cand> cand;
    std::future<Loaded> next;
    if (!steps.empty()) next = std::async(std::launch::async, load, steps[0].job);
    int phase = 1;
    int exit_code = 0;
    std::string fatal_message;
    for (size_t s = 0; s < steps.size(); s++) {
        const Step &st = steps[s];
        Loaded cur = next.get();
        if (s + 1 < steps.size() && cur.status == 0) next = std::async(std::launch::async, load, steps[s + 1].job);
        read_seconds += cur.seconds;
        while (phase < st.phase) { // blank line after each phase
            std::cout << std::endl;
            phase++;
        }
        std::cout << cur.could_not_find;
        const std::string &a = st.phase == 2 ? accession2[st.index] : accession[st.index];
        if (cur.status == 1) {
            std::cout << "no file for " << a << std::endl;
            exit_code = 1;
            break;
        }
        if (cur.status != 0) {
            exit_code = cur.status;
            fatal_message = cur.message;
            break;
        }
        const uint8_t *text = (const uint8_t *)cur.text.data();
        const uint64_t len = cur.text.size();
        std::cout << st.phase << " " << st.index << " " << (st.phase == 2 ? (int)accession2.size() : num_orgs) << " " << a << "\n";
        if (st.phase == 1) {
            check(kid_builder_add(b, text, len, targno[st.index]), "kid_builder_add");
        } else if (st.phase == 2) {
            check(kid_builder_remove(b, text, len), "kid_builder_remove");
        } else {
            // the host scan of process_seq2 (:553-640) over the first occurrences of live cells, in gpos order
            cand.resize(len > (uint64_t)(K - 1) ? len - (K - 1) : 1);
            uint64_t nc = 0;
            check(kid_builder_claim(b, text, len, 0, cand.data(), cand.size(), &nc), "kid_builder_claim");
            long minpos = -1;
            for (uint64_t c = 0; c < nc; c++) {
                const kid_build_cand &o = cand[c];
                if (o.gpos > minpos && pcount[o.target] < max_probes && (o.flags & 1)) {
                    const std::string km = kmer_text(o.key);
                    if (o.flags & 2) std::cout << km << std::endl;
                    out << km << "," << o.target << "," << st.index << "," << o.gpos << "," << (o.strand_r ? 'R' : 'F') << "," << o.count << "\n";
                    minpos = (long)o.gpos + K;
                    pcount[o.target]++;
                    tct++;
                }
            }
        }
    }
    if (exit_code == 0) {
        while (phase < 3) {
            std::cout << std::endl;
            phase++;
        }
        check(kid_builder_size(b, &size), "kid_builder_size"); // cells filled by phase 1 (phases 2 and 3 fill none)
    }
    out.close();
    if (exit_code != 0) {
        if (next.valid()) next.wait();
        kid_builder_destroy(b);
        std::cout.flush();
        if (!fatal_message.empty()) std::cerr << fatal_message << "\n";
        return exit_code;
    }
    std::cout << std::endl;
    {
        std::ofstream out2((wdir + name + "_count.txt").c_str());
        for (int i = 0; i < num_targ; i++) out2 << i << "," << pcount[i] << "\n";
    }
    std::cout << "probe count " << tct << std::endl;
    std::cout << "size " << size << std::endl;
    if (timing) {
        double ms[3];
        uint64_t bases[3];
        check(kid_builder_stats(b, ms, bases), "kid_builder_stats");
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
        char buf[512];
        snprintf(buf, sizeof(buf),
                 "{\"add_ms\": %.3f, \"remove_ms\": %.3f, \"claim_ms\": %.3f, \"add_bases\": %llu, \"remove_bases\": %llu, "
                 "\"claim_bases\": %llu, \"read_s\": %.3f, \"wall_s\": %.3f, \"size\": %llu, \"probes\": %ld}",
                 ms[0], ms[1], ms[2], (unsigned long long)bases[0], (unsigned long long)bases[1], (unsigned long long)bases[2], read_seconds,
                 wall, (unsigned long long)size, tct);
        std::cerr << buf << std::endl;
    }
    kid_builder_destroy(b);
    return 0;
}
