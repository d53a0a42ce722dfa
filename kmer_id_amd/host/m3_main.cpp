// kmer_read_m3 -- command-line compatible replacement of the reference's mitochondria reader, the
// back end of the Galaxy tool (kmer_read_m3.cpp, main at :973-1131):
//     kmer_read_m3 -wdir DIR/ -f1 reads1 [-f2 reads2|none]
// reads DIR/mitochondria_{data.txt,tree.txt,probes.txt.gz}, classifies -f1 and -f2
// (.fastq.gz / .fasta / .fastq / .fasta.gz) and writes DIR/result.txt.
// What reaches the kernel: lookups give up after MAXREPROBE = 16 probes (:42,:232), so the table is
// built sequentially on the host with the reference's exact cell geometry (results depend on it).
// Extra options: --k K (30) --log2-slots L (30) --device D (0) --batch-reads N
// and the side options (SideOptions, kid_side.h), whose files stand beside DIR/result.txt (SampleOutputs):
//   --hits   every read's k-mer hits
//   --min-hits N  --confidence F   the reads called by k-mer support
//   --segments LEN[:STEP]   long records called in segments
//   --segment-votes LEN[:STEP]   long records called in segments by root-path votes (the segment_votes file of kid_driver.h)
//   --loci W   every read with a hit placed on a genome by its colinear hits (the loci file of kid_driver.h)
//   --pileup W[:MIN_CHAIN[:MIN_MARGIN]]   the placed reads piled up per genome bin (the pileup file of kid_driver.h)
//   --depth   k-mer depth per target (the depth file of kid_driver.h)
//   --seen   the seen-bitmap in a seen file (<...>seen.bin beside <...>result.txt), for kmer_shared
//   --votes   the reads called by root-path votes, whatever the order of their hits (the votes file of kid_driver.h)
//   --min-base-quality Q   FASTQ bases of quality below Q (0..93; 0 = off) are read as N
//   --low-complexity T   bases in a low-complexity window at threshold T (0..1000; 0 = off, 20 = DUST's usual level) are read as N
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>

#include "kid_driver.h"

using namespace kidhost;

int main(int argc, char **argv)
{
    std::string wdir, r1name, r2name;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : "";
        if (a == "-wdir") wdir = v;
        if (a == "-f1") r1name = v;
        if (a == "-f2") r2name = v;
    }
    const ReaderOptions opt = parse_reader_options(argc, argv, /*threads=*/2);
    const int k = opt.k;
    const std::string iname = wdir + "mitochondria_data.txt", tname = wdir + "mitochondria_tree.txt",
                      pname = wdir + "mitochondria_probes.txt.gz";
    try {
        std::cout << "r1 " << r1name << std::endl;
        std::cout << "r2 " << r2name << std::endl;
        std::cout << "wd " << wdir << std::endl;
        int num_orgs = 0, num_targ = 0; // (num_targ is uninitialised in the reference, :981; 0 in practice)
        if (!count_strains(iname, num_orgs, num_targ)) {
            std::cerr << "kmer_read_m3: cannot read " << iname << "\n";
            return 3; // the reference builds a zero-sized tree here and crashes later
        }
        std::cout << num_orgs << " strains" << std::endl;
        {
            std::ifstream fin(tname);
            if (!fin) return 1; // `else exit(1)`, :1060
        }
        std::vector<int32_t> parent;
        ProbeSet ps;
        set_inflate_threads(opt.threads >= 6 ? opt.threads / 2 : 1); // (gzip inputs: pieces inflated side by side when there are threads for it)
        load_database(tname, pname, opt.db_cache, k, num_targ, parent, ps, nullptr, 0, nullptr, nullptr, (opt.side.loci.on || opt.side.pileup.on) && opt.dry_run.empty());
        std::cout << "tree loaded" << std::endl;
        std::cout << ps.lines_parsed << " kmers loaded" << std::endl;
        if (ps.lines_parsed < 2) return 1; // :1067

        // (a name without one of the four endings has no reader: an empty or 1-character -f2, "none", a missing -f1)
        const bool have2 = r2name.length() > 1 && r2name != "none";
        std::vector<std::string> names{r1name};
        if (have2) names.push_back(r2name);
        std::vector<char> missing;
        std::vector<SourceOpener> files = make_openers(names, k, missing);
        if (!opt.dry_run.empty()) return write_dry_run(opt.dry_run, "kmer_read_m3", parent, ps, names, files, opt.batch_reads, k);
        Engine eng;
        eng.batch_reads = opt.batch_reads;
        if (!engine_open(eng, ps, parent, k, opt.log2_slots, /*MAXREPROBE*/ 16, 0, parse_devices(opt.device, opt.device_list))) return 1;
        engine_configure(eng, opt.side);
        ps = ProbeSet();

        if (r1name.empty()) throw Fatal{134, "no -f1 given (std::out_of_range in the reference, :1080)"};
        std::cout << r1name.length() << " : " << r1name[r1name.length() - 1] << std::endl;
        Prefetcher pf(std::move(files), opt.threads, eng.batch_reads, eng.batch_bases);
        SampleOutputs outputs(wdir + "result.txt", opt.side);
        ReadSaver saver("", num_targ); // the reads file is commented out in this program (:612-621)
        auto is_fagz = [](const std::string &n) { return ends_with(n, ".fasta.gz"); };
        if (is_fagz(r1name)) std::cout << "true" << std::endl; // process_fagz, :789
        long long tct = run_files(eng, pf, 0, 1, saver, outputs, 0);
        if (missing[0]) std::cout << "nark " << r1name << std::endl;
        std::cout << tct << " reads loaded" << std::endl;
        if (have2) {
            if (is_fagz(r2name)) std::cout << "true" << std::endl;
            tct += run_files(eng, pf, 1, 1, saver, outputs, 1);
            if (missing[1]) std::cout << "nark " << r2name << std::endl;
            if (ends_with(r2name, ".fastq.gz")) std::cout << tct << " reads loaded" << std::endl; // printed inside that branch too (:1107)
            std::cout << tct << " reads loaded" << std::endl;
        }
        outputs.finish(eng);
        leave_now(0);
    } catch (const Fatal &f) {
        std::cerr << f.message << "\n";
        return f.exit_code;
    }
    return 0;
}
