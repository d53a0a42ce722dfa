// kmer_coverage -- breadth of coverage per organism, from the seen files that nk10 / kmer_read_vf6 / kmer_read_m3 --seen
// write and the org and position columns of the probes file:
//     kmer_coverage [--probes FILE(.gz) (./bact10/probes10.txt.gz)] [--k K (30)] [--bin-width W (1000)] [--device D (0)]
//                   [--threads T] [--min-seen M (1)] [--bins ORG] A_seen.bin B_seen.bin ...          (1..64 files)
// Where on its genome the database k-mers a sample saw lie (kid_seen_coverage: on the GPU, no table is built): an organism
// that is present is seen in nearly all of its bins of W bases, a conserved or contaminating region in a few of them.
// Order of work: the arguments; the files, whose headers must agree with each other and with --k; the probes with their
// sites, through the loader of the other front-ends, whose entry count must be the headers' n_entries; the GPU.  The
// number of organisms is the largest org of the probes file plus one.
// stdout, integers only: a line "#<index>\t<path>\t<bits set>" per file (the bits of its bitmap among the n_entries
// entries), then for file a in argument order and organisms ascending a line
//     a,org,n_probes,n_seen,span_bins,bins,bins_seen,max_gap,max_bin_seen,max_bin
// for every organism with n_seen >= M (the fields of kid_coverage, include/kmer_id_amd.h).  With --bins ORG those lines
// are replaced by a line "a,ORG,bin,probes,seen" for every occupied bin of that organism (kid_seen_coverage_bins).
// Exit codes: 2 usage (an unknown option, a missing or non-digit value, W = 0, no file or more than 64); 255 a file that
// cannot be opened; 3 a bad magic, a truncated file, headers that disagree, a probes file with another number of
// entries, a probe line without a site, an ORG the probes do not have, or an error of the library -- with one line on
// stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "kid_driver.h"

using namespace kidhost;

static int fail(int code, const std::string &what)
{
    std::cerr << "kmer_coverage: " << what << "\n";
    return code;
}

// digits only -> value (at most `max`); false otherwise
static bool number(const char *v, unsigned long long max, unsigned long long &out)
{
    if (!*v) return false;
    out = 0;
    for (; *v; v++) {
        if (*v < '0' || *v > '9') return false;
        out = out * 10 + (unsigned)(*v - '0');
        if (out > max) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    std::string probes = "./bact10/probes10.txt.gz";
    unsigned long long k = 30, width = 1000, device = 0, threads = 0, min_seen = 1, bins_org = 0;
    bool bins = false;
    std::vector<std::string> paths;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        struct { const char *name; unsigned long long *value, max; } const numbers[] = {
            {"--k", &k, 31}, {"--bin-width", &width, 0xFFFFFFFFull}, {"--device", &device, 1023}, {"--threads", &threads, 1024},
            {"--min-seen", &min_seen, 0xFFFFFFFFull}, {"--bins", &bins_org, 0xFFFFFFFFull}};
        bool taken = false;
        for (const auto &o : numbers) {
            if (a != o.name) continue;
            if (i + 1 >= argc) return fail(2, a + " needs a value");
            if (!number(argv[++i], o.max, *o.value)) return fail(2, a + " takes a number, digits only");
            if (o.value == &bins_org) bins = true;
            taken = true;
        }
        if (taken) continue;
        if (a == "--probes") {
            if (i + 1 >= argc) return fail(2, a + " needs a value");
            probes = argv[++i];
        } else if (a.size() > 1 && a[0] == '-' && a[1] == '-') {
            return fail(2, "unknown option " + a);
        } else {
            paths.push_back(a);
        }
    }
    if (paths.empty() || paths.size() > KID_SHARED_MAX_SAMPLES || k < 1 || width < 1)
        return fail(2, "usage: kmer_coverage [--probes FILE] [--k K] [--bin-width W (>= 1)] [--device D] [--threads T] [--min-seen M] "
                       "[--bins ORG] A_seen.bin B_seen.bin ...   (1..64 files)");

    // ---- the files: header and bitmap of each
    const size_t n = paths.size();
    std::vector<std::vector<uint8_t>> maps;
    SeenHeader first;
    {
        std::string what;
        const int code = read_seen_files(paths, -1, k, maps, first, what);
        if (code != 0) return fail(code, what);
    }

    try {
        // ---- the probes: organism and position of the entries in file order
        set_inflate_threads(threads >= 6 ? (int)threads / 2 : 1);
        const ProbeSet ps = load_probes_gz(probes, (int)k, (int)threads, nullptr, /*want_sites=*/true);
        if (ps.targets.size() != first.n_entries)
            return fail(3, probes + " has " + std::to_string(ps.targets.size()) + " entries, the seen files were written for " +
                               std::to_string(first.n_entries));
        const uint64_t n_entries = first.n_entries;
        uint64_t n_orgs = 0;
        for (uint64_t o = 0; o < n_entries; o++)
            if ((uint64_t)ps.orgs[o] + 1 > n_orgs) n_orgs = (uint64_t)ps.orgs[o] + 1;
        if (n_orgs > 0xFFFFFFFFull) return fail(3, probes + " names organism 4294967295: one more than the library counts");
        if (bins && bins_org >= n_orgs)
            return fail(3, "--bins " + std::to_string(bins_org) + ": " + probes + " has the organisms 0.." + std::to_string((long long)n_orgs - 1));
        // ---- the GPU
        std::vector<const void *> ptrs(n);
        for (size_t f = 0; f < n; f++) ptrs[f] = maps[f].data();
        std::string out;
        char line[200];
        if (!bins) {
            std::vector<kid_coverage> recs(n * (size_t)n_orgs);
            const int rc = kid_seen_coverage((int)device, ps.orgs.data(), ps.positions.data(), n_entries, (uint32_t)n_orgs, (uint32_t)width,
                                             ptrs.data(), (int)n, recs.data());
            if (rc != KID_OK) return fail(3, std::string(kid_strerror(rc)) + ": " + kid_last_error());
            for (size_t f = 0; f < n; f++) {
                unsigned long long bits = 0;
                for (size_t g = 0; g < n_orgs; g++) bits += recs[f * n_orgs + g].n_seen;
                out += "#" + std::to_string(f) + "\t" + paths[f] + "\t" + std::to_string(bits) + "\n";
            }
            for (size_t f = 0; f < n; f++)
                for (size_t g = 0; g < n_orgs; g++) {
                    const kid_coverage &r = recs[f * n_orgs + g];
                    if (r.n_seen < min_seen) continue;
                    const int len = snprintf(line, sizeof(line), "%zu,%zu,%u,%u,%u,%u,%u,%u,%u,%u\n", f, g, r.n_probes, r.n_seen, r.span_bins,
                                             r.bins, r.bins_seen, r.max_gap, r.max_bin_seen, r.max_bin);
                    out.append(line, (size_t)len);
                }
        } else {
            std::vector<uint64_t> base((size_t)n_orgs + 1);
            uint64_t B = 0;
            int rc = kid_seen_coverage_bins((int)device, ps.orgs.data(), ps.positions.data(), n_entries, (uint32_t)n_orgs, (uint32_t)width,
                                            ptrs.data(), (int)n, base.data(), nullptr, nullptr, 0, &B);
            if (rc != KID_OK) return fail(3, std::string(kid_strerror(rc)) + ": " + kid_last_error());
            std::vector<uint32_t> probes_per_bin((size_t)B), seen_per_bin(n * (size_t)B);
            rc = kid_seen_coverage_bins((int)device, ps.orgs.data(), ps.positions.data(), n_entries, (uint32_t)n_orgs, (uint32_t)width, ptrs.data(),
                                        (int)n, base.data(), probes_per_bin.data(), seen_per_bin.data(), B, &B);
            if (rc != KID_OK) return fail(3, std::string(kid_strerror(rc)) + ": " + kid_last_error());
            for (size_t f = 0; f < n; f++) {
                unsigned long long bits = 0;
                for (size_t b = 0; b < B; b++) bits += seen_per_bin[f * B + b];
                out += "#" + std::to_string(f) + "\t" + paths[f] + "\t" + std::to_string(bits) + "\n";
            }
            for (size_t f = 0; f < n; f++)
                for (uint64_t b = base[bins_org]; b < base[bins_org + 1]; b++) {
                    if (probes_per_bin[b] == 0) continue;
                    const int len = snprintf(line, sizeof(line), "%zu,%llu,%llu,%u,%u\n", f, bins_org, (unsigned long long)(b - base[bins_org]),
                                             probes_per_bin[b], seen_per_bin[f * B + b]);
                    out.append(line, (size_t)len);
                }
        }
        fwrite(out.data(), 1, out.size(), stdout);
        leave_now(0);
    } catch (const Fatal &f) {
        std::cerr << f.message << "\n";
        return f.exit_code;
    }
    return 0;
}
