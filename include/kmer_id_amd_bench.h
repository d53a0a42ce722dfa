/* kmer_id_amd_bench.h -- what bench.py, the tests and tools/ need beside the boundary (kmer_id_amd.h): the seeded
 * synthetic workload (DESIGN.md "synthetic workload"), the random-line probe the kernel is priced against, and plain
 * device memory helpers for host languages without a HIP binding.  Exported by the same library.                    */
#ifndef KMER_ID_AMD_BENCH_H
#define KMER_ID_AMD_BENCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
struct kid_db;
struct kid_sample;
/* ---- synthetic workload generators (bench + tests; deterministic, seeded) ------
 * DB key j = canonical(splitmix64(seed + j) mod 4^k); target of key j follows
 * cum[] (cum[t] <= j < cum[t+1]).  Reads: see DESIGN.md "synthetic workload".    */
int kid_synth_db_keys_host(uint64_t seed, int k, const uint64_t *cum, int32_t ntar,
                           uint64_t j0, uint64_t n, uint64_t *keys, uint32_t *targets);
int kid_synth_db_keys_device(uint64_t seed, int k, const uint64_t *cum_host, int32_t ntar,
                             uint64_t j0, uint64_t n, void *d_keys, void *d_targets, int device);
int kid_synth_reads_host(uint64_t db_seed, uint64_t read_seed, int k, const uint64_t *cum,
                         const int32_t *parent, int32_t ntar, uint64_t r0, uint64_t n_reads,
                         uint32_t read_len, uint8_t *bases);
int kid_synth_reads_device(uint64_t db_seed, uint64_t read_seed, int k, const uint64_t *cum_host,
                           const int32_t *parent_host, int32_t ntar, uint64_t r0, uint64_t n_reads,
                           uint32_t read_len, void *d_bases, int device);

/* random gather micro-benchmark over the DB's own table: the measured ceiling the
 * lookup kernel is priced against.  inflight = 101 / 108: random 128-byte LINES,
 * one 16-byte load per lane as the classify kernel issues it (64 distinct lines per
 * load / runs of 8 lanes on a line), four loads in flight per lane; *loads_out = the
 * distinct line requests of one launch.  inflight = 1,2,4,8: n_loads random cells,
 * that many independent loads per lane, of which the compiler keeps two 4-byte
 * loads per cell (the round-1 probe: twice the load instructions per line, it tops
 * out at 39 G cells/s where the line probe reaches 49 G lines/s).
 * inflight = 201 / 208: the shapes of 101 / 108 on the table's digest plane, one 8-byte
 * load per lane (KID_ERR_ARG for a table without a plane).
 * *ms_out = milliseconds per launch.                                               */
int kid_bench_gather(struct kid_db *db, uint64_t n_loads, int inflight, int iters, float *ms_out, uint64_t *loads_out);

/* where the table and its digest plane (8 bytes per 128-byte line; none: null and 0) lie in device memory, for
 * kid_dev_download: tests recompute the plane from the table's headers */
int kid_bench_db_arrays(struct kid_db *db, const void **table, uint64_t *table_bytes, const void **digest, uint64_t *digest_bytes);

/* which kid_classify_kernel instantiations the sample has launched since it began or was last reset: bit
 * PAIRK*16 | ROWS<<3 | HIST<<2 | MINLOC<<1 | (KFIX == 30) per instantiation (PAIRK 1 pair loop, 2 duo loop, 0 general
 * loops).  A launch is recorded whether or not the kernel finds work: a batch with device-side offsets launches all
 * three loops of its configuration, and the two the batch is not for return at once.  The DIGEST instantiations of
 * the pair and duo loops (KID_OPT_LINE_DIGEST) have bits of their own: 48 + (PAIRK - 1)*8 + (ROWS<<2 | HIST<<1 |
 * (KFIX == 30)).                                                                                                      */
int kid_sample_kernel_variants(struct kid_sample *s, uint64_t *mask);

/* the state of the sample's hit log, for tests that must prove which regime they reached.  Synchronises the device; reads
 * only: the log is not applied, and neither the pacing of the passes nor any counter changes.
 *   passes   passes over the log queued since the sample began or was last reset (by the pace or by a reader)
 *   has_log  the sample has a log at all (minimizer-localised table, bitmap of at most 1024 pieces)
 *   logging  has_log and no pass has switched the log off: the device's own word, as of the synchronise          */
int kid_sample_log_state(struct kid_sample *s, uint32_t *passes, int *has_log, int *logging);

/* the share of kid_seen_coverage_time that the count kernels over the bitmaps took (the hot pass: without the span
 * stage, the probes per bin and the reduce kernels), in this process, since the last query                          */
int kid_bench_coverage_count_time(double *count_ms);

/* device memory helpers so that a host language without a HIP binding can stage buffers */
int kid_dev_alloc(int device, uint64_t nbytes, void **d_ptr);
int kid_dev_free(int device, void *d_ptr);
int kid_dev_upload(int device, void *d_dst, const void *src, uint64_t nbytes);
int kid_dev_download(int device, void *dst, const void *d_src, uint64_t nbytes);
int kid_dev_sync(int device);

#ifdef __cplusplus
}
#endif
#endif /* KMER_ID_AMD_BENCH_H */
