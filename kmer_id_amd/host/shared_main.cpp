// kmer_shared -- k-mers shared between samples, from the seen files that nk10 / kmer_read_vf6 / kmer_read_m3 --seen write:
//     kmer_shared [--probes FILE(.gz) (./bact10/probes10.txt.gz)] [--ntar N (5982)] [--k K (30)] [--device D (0)]
//                 [--threads T] [--min-shared M (0)] A_seen.bin B_seen.bin ...          (1..64 files)
// For every pair of files and every target: how many of the target's database k-mers both samples saw
// (kid_shared_kmers: one pass on the GPU for all pairs, no table is built).  Order of work: the arguments; the files,
// whose headers must agree with each other and with --ntar / --k; the probes, through the loader of the other
// front-ends, whose entry count must be the headers' n_entries; the GPU.
// stdout, integers only: a line "#<index>\t<path>\t<bits set>" per file (the bits of its bitmap among the n_entries
// entries), then for a < b in argument order and targets ascending a line "a,b,target,kmers_a,kmers_b,shared" for every
// target with kmers_a > 0, kmers_b > 0 and shared >= M; kmers_x is the file's own number of bits under the target.
// Exit codes: 2 usage; 255 a file that cannot be opened; 3 a bad magic, a truncated file, headers that disagree, or an
// error of the library -- with one line on stderr.
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
    std::cerr << "kmer_shared: " << what << "\n";
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
    unsigned long long ntar = 5982, k = 30, device = 0, threads = 0, min_shared = 0;
    std::vector<std::string> paths;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        struct { const char *name; unsigned long long *value, max; } const numbers[] = {
            {"--ntar", &ntar, 0x7FFFFFFFull}, {"--k", &k, 31}, {"--device", &device, 1023}, {"--threads", &threads, 1024},
            {"--min-shared", &min_shared, ~0ull >> 1}};
        bool taken = false;
        for (const auto &o : numbers) {
            if (a != o.name) continue;
            if (i + 1 >= argc) return fail(2, a + " needs a value");
            if (!number(argv[++i], o.max, *o.value)) return fail(2, a + " takes a number, digits only");
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
    if (paths.empty() || paths.size() > KID_SHARED_MAX_SAMPLES || ntar < 1 || k < 1)
        return fail(2, "usage: kmer_shared [--probes FILE] [--ntar N] [--k K] [--device D] [--threads T] [--min-shared M] "
                       "A_seen.bin B_seen.bin ...   (1..64 files)");

    // ---- the files: header and bitmap of each
    const size_t n = paths.size();
    std::vector<std::vector<uint8_t>> maps;
    SeenHeader first;
    {
        std::string what;
        const int code = read_seen_files(paths, (long long)ntar, k, maps, first, what);
        if (code != 0) return fail(code, what);
    }

    try {
        // ---- the probes: the targets of the entries in file order
        set_inflate_threads(threads >= 6 ? (int)threads / 2 : 1);
        const ProbeSet ps = load_probes_gz(probes, (int)k, (int)threads);
        if (ps.targets.size() != first.n_entries)
            return fail(3, probes + " has " + std::to_string(ps.targets.size()) + " entries, the seen files were written for " +
                               std::to_string(first.n_entries));
        // ---- the GPU
        std::vector<const void *> ptrs(n);
        for (size_t f = 0; f < n; f++) ptrs[f] = maps[f].data();
        std::vector<int64_t> shared(n * n * (size_t)ntar);
        const int rc = kid_shared_kmers((int)device, ps.targets.data(), first.n_entries, (int32_t)ntar, ptrs.data(), (int)n, 0, shared.data());
        if (rc != KID_OK) return fail(3, std::string(kid_strerror(rc)) + ": " + kid_last_error());
        auto at = [&](size_t a, size_t b, size_t t) { return shared[(a * n + b) * (size_t)ntar + t]; };
        std::string out;
        for (size_t f = 0; f < n; f++) {
            long long bits = 0;
            for (size_t t = 0; t < ntar; t++) bits += at(f, f, t);
            out += "#" + std::to_string(f) + "\t" + paths[f] + "\t" + std::to_string(bits) + "\n";
        }
        char line[160];
        for (size_t a = 0; a < n; a++)
            for (size_t b = a + 1; b < n; b++)
                for (size_t t = 0; t < ntar; t++) {
                    const long long ka = at(a, a, t), kb = at(b, b, t), s = at(a, b, t);
                    if (ka <= 0 || kb <= 0 || (unsigned long long)s < min_shared) continue;
                    const int len = snprintf(line, sizeof(line), "%zu,%zu,%zu,%lld,%lld,%lld\n", a, b, t, ka, kb, s);
                    out.append(line, (size_t)len);
                }
        fwrite(out.data(), 1, out.size(), stdout);
        leave_now(0);
    } catch (const Fatal &f) {
        std::cerr << f.message << "\n";
        return f.exit_code;
    }
    return 0;
}
