// kmer_read_vf6 -- command-line compatible replacement of the reference's generic reader
// (kmer_read_vf6.cpp, main at :968-1170):
//     kmer_read_vf6 -name DB -jname JOBS [-target T] [-fadir DIR]
// reads ./DB/DB_data.txt, ./DB/DB_tree.txt, ./DB/DB_probes.txt.gz and the job list
// ./JOBS/JOBS.txt ("<job> <nfiles>" followed by nfiles paths), classifies every file of a job
// (.fastq.gz / .fasta.gz / .fasta / .fastq) on the GPU and writes ./JOBS/<job>_result.txt,
// ./JOBS/<job>_reads.txt and, with -target, ./JOBS/<job>_target_reads.txt.
// Differences to nk10 that reach the kernel: U/u count as T (:496-500,521-525) and the number of
// targets comes from the data file (:1073-1084).
// Extra options: --k K (30) --log2-slots L (30) --device D (0) --batch-reads N
// and the side options (SideOptions, kid_side.h), whose files stand beside ./JOBS/<job>_result.txt (SampleOutputs):
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

#include <iostream>

#include "kid_driver.h"

using namespace kidhost;

int main(int argc, char **argv)
{
    std::string dname, wdir, jname, jdir, fdir;
    int save_target = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : "";
        if (a == "-name") { dname = v; wdir = "./" + dname + "/"; }
        if (a == "-fadir") fdir = v; // only the dead alignment branch reads it
        if (a == "-jname") { jname = v; jdir = "./" + jname + "/"; }
        if (a == "-target") save_target = atoi(v);
    }
    const ReaderOptions opt = parse_reader_options(argc, argv, /*threads=*/4);
    const int k = opt.k;
    const std::string iname = wdir + dname + "_data.txt", tname = wdir + dname + "_tree.txt",
                      pname = wdir + dname + "_probes.txt.gz", jfile = jdir + jname + ".txt";
    try {
        // ---- job list (:1021-1057)
        JobList jobs;
        if (load_job_list(jfile, jobs)) std::cout << jobs.runnable << " jobs" << std::endl;
        else std::cout << "narin " << jfile << std::endl;
        // ---- strain list: number of targets = largest target id + 1 (:1059-1089)
        int num_orgs = 0, num_targ = 0;
        if (!count_strains(iname, num_orgs, num_targ)) {
            std::cout << "narin " << iname << std::endl;
            std::cerr << "kmer_read_vf6: no strain list, the number of targets is unknown\n";
            return 3; // the reference goes on with a zero-sized tree and crashes
        }
        std::cout << num_orgs << " strains" << std::endl;
        std::cout << num_targ - 1 << " targs" << std::endl;
        std::vector<int32_t> parent;
        ProbeSet ps;
        set_inflate_threads(opt.threads >= 6 ? opt.threads / 2 : 1); // (gzip inputs: pieces inflated side by side when there are threads for it)
        load_database(tname, pname, opt.db_cache, k, num_targ, parent, ps, nullptr, 0, nullptr, nullptr, (opt.side.loci.on || opt.side.pileup.on) && opt.dry_run.empty());
        std::cout << "tree loaded" << std::endl;
        std::cout << ps.lines_parsed << " kmers loaded" << std::endl;

        std::vector<std::string> names, labels;
        for (int j = 0; j < jobs.runnable; j++)
            for (int i = 0; i < jobs.n_inputs(j); i++) {
                names.push_back(jobs.file_rows[(size_t)j][(size_t)i]);
                labels.push_back(jobs.header_name[(size_t)j] + " " + names.back());
            }
        std::vector<char> missing;
        std::vector<SourceOpener> files = make_openers(names, k, missing);
        if (!opt.dry_run.empty()) return write_dry_run(opt.dry_run, "kmer_read_vf6", parent, ps, labels, files, opt.batch_reads, k);
        Engine eng;
        eng.batch_reads = opt.batch_reads;
        if (!engine_open(eng, ps, parent, k, opt.log2_slots, 0, KID_FLAG_U_IS_T, parse_devices(opt.device, opt.device_list))) return 1;
        engine_configure(eng, opt.side);
        ps = ProbeSet();

        Prefetcher pf(std::move(files), opt.threads, eng.batch_reads, eng.batch_bases);
        size_t fi = 0;
        for (int j = 0; j < jobs.runnable; j++) { // :1116-1164
            const std::string jstr = jobs.header_name[(size_t)j];
            engine_reset(eng);
            const std::string base = "./" + jname + "/" + jstr;
            long long tct = 0;
            SampleOutputs outputs(base + "_result.txt", opt.side);
            {
                ReadSaver saver(base + "_reads.txt", num_targ, save_target > 0 ? base + "_target_reads.txt" : "",
                                (uint32_t)(save_target > 0 ? save_target : 0), save_target == 0);
                for (int i = 0; i < jobs.n_inputs(j); i++, fi++) {
                    std::cout << names[fi] << std::endl;
                    tct += run_files(eng, pf, fi, 1, saver, outputs, (size_t)i);
                    if (missing[fi]) std::cout << "nark " << names[fi] << std::endl;
                }
            }
            std::cout << tct << " reads loaded" << std::endl;
            outputs.finish(eng);
        }
        leave_now(0);
    } catch (const Fatal &f) {
        std::cerr << f.message << "\n";
        return f.exit_code;
    }
    return 0;
}
