/*
 * kmer_id_amd.h -- C ABI of libkmer_id_amd.so, the MI355X (gfx950) k-mer read
 * classifier.  This is the drop-in boundary for the hot path of
 * mmammel8/kmer_id: everything `process_read` (newkmer_10nx.cpp:452-617) does
 * with the global hash table `ht` (:158-266), the global taxonomy `taxonomy`
 * (:93-156) and the global counters `gcount/ucount/kmer_seen` (:61-64).
 *
 * The reference has no FFI of its own (it is one translation unit with global
 * state), so each entry point below names the reference code it replaces.
 * INTEGRATION.md shows the ~40-line patch that makes newkmer_10nx.cpp call
 * these instead of its own loop.
 *
 * Conventions: plain C types only; every function returns KID_OK (0) or a
 * negative kid_status; no exception crosses the boundary; the caller owns every
 * buffer it passes; the library owns the handles until *_destroy.  There is NO
 * CPU fallback: without a HIP device every compute entry point returns
 * KID_ERR_NO_DEVICE.
 */
#ifndef KMER_ID_AMD_H
#define KMER_ID_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum kid_status {
    KID_OK = 0,
    KID_ERR_ARG = -1,        /* bad argument (null pointer, size, offsets not monotone, start/stop outside read) */
    KID_ERR_NOMEM = -2,      /* host or device allocation failed */
    KID_ERR_HIP = -3,        /* a HIP runtime call failed; see kid_last_error() */
    KID_ERR_TABLE_FULL = -4, /* more than 2^log2_slots - 32 entries: the reference prints
                                "out of memory in table" and exit(1)s, newkmer_10nx.cpp:256-260 */
    KID_ERR_TREE = -5,       /* parent[] has an out-of-range entry or a cycle (the reference would loop forever in msca) */
    KID_ERR_NO_DEVICE = -6,  /* no usable HIP device */
    KID_ERR_TARGET = -7,     /* a target id >= ntar (the reference would index gcount[] out of bounds) */
    KID_ERR_IO = -8,         /* file could not be opened / gz error (reference: exit(255), newkmer_10nx.cpp:87-91) */
    KID_ERR_FORMAT = -9,     /* input line >= 16 KiB (exit 255, :773) or qual shorter than seq (std::out_of_range, :727) */
    KID_ERR_STATE = -10      /* call sequence error (e.g. classify after sample_end without reset) */
} kid_status;

/* option bits for kid_db_build*() */
#define KID_FLAG_U_IS_T 1u    /* U/u is read as T: kmer_read_vf6.cpp:496-500,521-525 */
#define KID_FLAG_HOST_BUILD 2u /* build the table on the host with the reference's sequential insert
                                  order (exact cell geometry).  Implied when max_probes > 0. */
#define KID_FLAG_REF_GEOMETRY 4u /* GPU build, but with the reference's cell placement (fmix64 +
                                  triangular probing) instead of the minimizer-localised one.  Lookup
                                  results are the same either way; only speed differs. */

typedef struct kid_db kid_db;         /* hash table + taxonomy, resident in one GPU's HBM */
typedef struct kid_sample kid_sample; /* per-sample counters: gcount, seen-bitmap (-> ucount) */

typedef struct kid_db_info {
    int32_t ntar;        /* number of taxonomy nodes (MAXTAR, newkmer_10nx.cpp:45) */
    int32_t k;           /* k-mer length (KSIZE, :43) */
    int32_t log2_slots;  /* log2 of the table size (MAXHASH, :49) */
    int32_t max_probes;  /* 0 = unbounded (10nx, vf6); 16 = kmer_read_m3.cpp:42,232 */
    uint32_t flags;
    int32_t device;
    int32_t tree_depth;  /* deepest node (root = 0) */
    int32_t host_built;  /* 1 if the sequential host builder produced the table */
    int32_t geometry;    /* 0 = reference placement, 1 = minimizer-localised placement */
    int32_t reserved_;
    uint64_t n_entries;  /* entries handed to the builder */
    uint64_t n_occupied; /* cells with value != 0 */
    uint64_t table_bytes;
} kid_db_info;

const char *kid_strerror(int status);
const char *kid_last_error(void); /* thread-local detail of the last failure */
int kid_device_count(int *count);

/* ---- database ------------------------------------------------------------
 * Replaces: Hashtable::Hashtable + HashClear + add_kmer (newkmer_10nx.cpp:173-180,
 * 199-202, 235-263) and Tree1::Tree1 + add_edge (:101-116).
 *   keys[i], targets[i]  the forward 2-bit keys and target ids in probes-file
 *                        order, exactly what process_kmer (:619-661) hands to
 *                        add_kmer; duplicates allowed, first one wins on lookup.
 *   parent[ntar]         Tree1::parent after all add_edge calls (default 1 = root).
 *   k                    KSIZE (1..31);  log2_slots  log2(MAXHASH) (6..32: slot indices are 32-bit)
 *   n                    at most 2^32-2 entries and at most 2^log2_slots - 32 (KID_ERR_TABLE_FULL beyond, like
 *                        the reference); the minimizer-localised placement is used while n <= 80 % of the cells
 *   max_probes           0 or the MAXREPROBE of kmer_read_m3.cpp
 *   device               HIP device ordinal
 * Table cells are 16 B {u64 key, u32 target, u32 insertion ordinal+1}.           */
int kid_db_build(const uint64_t *keys, const uint32_t *targets, uint64_t n,
                 const int32_t *parent, int32_t ntar, int k, int log2_slots,
                 int max_probes, uint32_t flags, int device, kid_db **out);
/* same, keys/targets already resident on `device` (used by the synthetic bench DB) */
int kid_db_build_device(const void *d_keys, const void *d_targets, uint64_t n,
                        const int32_t *parent, int32_t ntar, int k, int log2_slots,
                        int max_probes, uint32_t flags, int device, kid_db **out);
/* a replica of `src` in the HBM of `device` (device-to-device copies; the reference, pinned into every GPU) */
int kid_db_replicate(const kid_db *src, int device, kid_db **out);
int kid_db_get_info(const kid_db *db, kid_db_info *out);
void kid_db_destroy(kid_db *db);

/* Hashtable::getHash (newkmer_10nx.cpp:204-233) for a batch of keys, on the GPU.
 * probes (nullable) receives the number of cells each lookup read. */
int kid_db_lookup(kid_db *db, const uint64_t *keys, uint64_t n, uint32_t *targets, uint32_t *probes);
/* Hashtable::integerHash (newkmer_10nx.cpp:189-197, MurmurHash3 fmix64) for a batch of keys, computed by the
 * device code that places and finds the cells of the reference geometry. */
int kid_hash_keys(int device, const uint64_t *keys, uint64_t n, uint64_t *out);
/* Tree1::msca (newkmer_10nx.cpp:118-144) for a batch of (x,y), on the GPU. */
int kid_db_msca(kid_db *db, const int32_t *x, const int32_t *y, uint64_t n, int32_t *out);

/* ---- per-sample state ----------------------------------------------------
 * Replaces the per-sample reset in main (newkmer_10nx.cpp:1017-1019,1023).   */
int kid_sample_begin(kid_db *db, kid_sample **out);
/* options of a sample */
#define KID_OPT_INPUTS_READY 1 /* value 1: the read text handed to kid_classify_batch_device / kid_classify_fixed_device is
                                  final when the call is made and stays untouched until the batch is through (e.g. batches
                                  resident in HBM): the library may then pack a batch on a stream of its own while the batch
                                  before is still being classified, instead of strictly behind it in `stream` */
#define KID_OPT_LONG_RECORD_KMERS 2 /* value: records of more k-mers than this (default 65536; 0 = never) are classified by
                                      the long-record kernels -- every k-mer looked up by a lane of its own, one ordered
                                      fold per record -- instead of by one wavefront (FASTA contigs, kmer_read_vf6.cpp:803-861) */
#define KID_OPT_MIN_BASE_QUALITY 3 /* value Q in 0..93 (KID_ERR_ARG beyond), 0 = off (the default): the FASTQ blocks handed to
                                     kid_classify_fastq_async after the call have every base of quality below Q read as 'N'
                                     ("mask low-quality bases" below).  Like the other options it stays until it is set again;
                                     kid_sample_reset does not change it */
#define KID_OPT_ENTRY_DEPTH 4 /* value 1: the sample gets one uint32 counter per database entry, zeroed ("k-mer depth per
                                database entry" below); setting 1 again while it is on changes nothing.  value 0 frees the
                                counters and loses the counts.  Any other value is KID_ERR_ARG.  kid_sample_reset zeroes the
                                counters and leaves the option on */
#define KID_OPT_LOW_COMPLEXITY 5 /* value T in 0..1000 (KID_ERR_ARG beyond), 0 = off (the default): the FASTQ blocks handed to
                                   kid_classify_fastq_async after the call have every base of a low-complexity window read
                                   as 'N' ("mask low-complexity sequence" below; T = 20 is DUST's usual level).  It stays
                                   until it is set again; kid_sample_reset does not change it */
#define KID_OPT_LINE_DIGEST 6 /* which front half the pair and duo loops (reads of up to 256 k-mers) run on a GPU-built
                                minimizer-localised table: 0 = they read the table's line headers, 1 = the 8-byte line digests
                                of the plane beside the table, 2 = auto (the default): digests until a pass over the hit log
                                finds the sample's reads full of hits, then headers until kid_sample_reset.  Results are the
                                same either way; only stats.probes may differ.  Any other value is KID_ERR_ARG.  A table
                                without a plane (reference geometry, host-built) takes the headers whatever the value */
int kid_sample_set_option(kid_sample *s, int option, int value);
int kid_sample_reset(kid_sample *s);
void kid_sample_destroy(kid_sample *s);

/* ---- classification (THE hot path) -----------------------------------------
 * Replaces process_read (newkmer_10nx.cpp:452-617) for n_reads reads at once.
 *   bases     ASCII read text, all reads concatenated (any bytes; only ACGTacgt,
 *             and Uu with KID_FLAG_U_IS_T, extend a k-mer: :478-525)
 *   offsets   n_reads+1 byte offsets into bases (read r = [offsets[r], offsets[r+1]))
 *   start/stop  inclusive range inside each read, as computed by process_qual
 *             (:714-760); pass NULL/NULL for whole reads (the FASTA callers, :851)
 *   out_final_targ  nullable; receives process_read's return value per read
 * Side effects on the sample: gcount[final_targ]++ per read (:613), and every
 * k-mer hit with target > 1 marks its DB entry as seen (:596-603).
 * Reads are independent; results do not depend on batch boundaries.  A batch
 * holds at most 2^31-1 reads (KID_ERR_ARG beyond; split the batch).           */
int kid_classify_batch(kid_sample *s, const uint8_t *bases, const uint64_t *offsets,
                       const int32_t *start, const int32_t *stop, uint64_t n_reads,
                       uint32_t *out_final_targ);
/* The same, asynchronous: returns once the batch has been queued -- its upload (a copy stream), its kernels (the
 * sample's stream) and the download of out_final_targ (a result stream) overlap with those of the batches before and
 * after it; up to three batches are in flight, a fourth call waits for the oldest.  The caller's buffers (inputs AND
 * out_final_targ) belong to the library until kid_classify_wait(ticket) returns.  Buffers from kid_host_alloc (pinned)
 * are transferred by DMA straight from / to the caller's memory; pageable ones work too but are staged by the HIP
 * runtime.  This replaces the reader loop of process_fqgz (newkmer_10nx.cpp:762-816) handing reads to process_read one
 * at a time.  kid_sample_end waits for everything in flight.                                                     */
int kid_classify_batch_async(kid_sample *s, const uint8_t *bases, const uint64_t *offsets,
                             const int32_t *start, const int32_t *stop, uint64_t n_reads,
                             uint32_t *out_final_targ, uint64_t *ticket);
/* fixed-length whole reads laid out back to back in host memory (no offsets array to upload) */
int kid_classify_fixed_async(kid_sample *s, const uint8_t *bases, uint32_t read_len, uint64_t n_reads,
                             uint32_t *out_final_targ, uint64_t *ticket);
/* A block of FASTQ text, asynchronous like kid_classify_batch_async: the caller has only FOUND the lines (the part of
 * process_fqgz, newkmer_10nx.cpp:762-816, that is inflate + splitting at '\n'); process_qual (:714-760), its
 * "stop - start >= 30" test (:757) and process_read run on the GPU for every record.
 *   text[text_nbytes]  the block as it came out of the file (< 4 GiB); recs[r] = byte offsets / lengths of the sequence
 *                      line and the quality line of record r (without '\n' / '\r')
 *   out_start/out_stop what process_qual computed; the reference hands the read to process_read iff stop - start >= k
 *                      -- records that fail the test are counted nowhere (gcount, ucount and "reads loaded" do not see
 *                      them) and get out_final_targ = 0
 * A quality line shorter than its sequence (std::out_of_range in the reference, :727) is reported as KID_ERR_FORMAT
 * by kid_sample_end / kid_sample_gcount.                                                                        */
typedef struct kid_fastq_rec {
    uint32_t seq_off, seq_len, qual_off, qual_len;
} kid_fastq_rec;
int kid_classify_fastq_async(kid_sample *s, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs,
                             uint64_t n_reads, uint32_t *out_final_targ, int32_t *out_start, int32_t *out_stop, uint64_t *ticket);
int kid_classify_wait(kid_sample *s, uint64_t ticket);
/* pinned (page-locked) host memory for the buffers above, placed on the NUMA node `device` is attached to */
int kid_host_alloc(int device, uint64_t nbytes, void **ptr);
int kid_host_free(void *ptr);
/* Device-resident form, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 *   d_bases    the ASCII read text in HBM; the classify kernels read it AS IT IS (there is no packed copy): it must be
 *              16-byte aligned, its allocation must extend at least 16 bytes past bases_nbytes (= offsets[n_reads]), and it
 *              must stay untouched until the batch is through -- i.e. until everything queued on `stream` up to this
 *              call has run, not just until the call returns
 *   d_offsets, d_start, d_stop  read by a small kernel in front of the classify kernels (read descriptors, range checks);
 *              the same lifetime.  The library keeps three sets of descriptor scratch and uses them in turn; the classify
 *              kernels of a sample's batches never overlap each other (batches handed over on different streams are ordered
 *              behind each other by an event wait).  Under KID_OPT_INPUTS_READY the descriptor kernel of batch b + 1 may
 *              run while batch b is being classified.
 *   Records of more than KID_OPT_LONG_RECORD_KMERS k-mers are sorted out on the device and take the long-record kernels. */
int kid_classify_batch_device(kid_sample *s, const void *d_bases, uint64_t bases_nbytes,
                              const void *d_offsets, const void *d_start, const void *d_stop,
                              uint64_t n_reads, void *d_out_final_targ, void *stream);
/* Fixed-length reads laid out back to back (read r = bases[r*read_len, (r+1)*read_len)), whole reads, no offsets
 * array: the layout of the synthetic roofline runs.  One kernel launch per batch (no descriptors, nothing in front of
 * the classify kernel); the same alignment / lifetime rules for d_bases.                                            */
int kid_classify_fixed_device(kid_sample *s, const void *d_bases, uint32_t read_len,
                              uint64_t n_reads, void *d_out_final_targ, void *stream);

/* process_qual (newkmer_10nx.cpp:714-760) for a batch: quals laid out like bases.
 * keep[r] = 1 if the reference would call process_read (stop-start >= k).        */
int kid_trim_batch(kid_db *db, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads,
                   int32_t *start, int32_t *stop, uint8_t *keep);

/* ---- mask low-quality bases -----------------------------------------------------------
 * process_qual lets the quality line decide only how much of each END of a read is cut off: a Q2 base in the middle of a
 * read takes part in 30 k-mers like any other.  With a minimum base quality Q (1..93; 0 = off, nothing runs) and
 * T = Q + 33, base i (0 <= i < seq_len) of a FASTQ record with qual_len >= seq_len is MASKED when its quality byte, read
 * as signed char exactly as process_qual reads it, is < T -- so bytes >= 128 are masked.  Quality bytes beyond seq_len are
 * ignored; the whole sequence line is covered, not only the trimmed range; a masked base behaves in every respect like a
 * byte that is not ACGTacgt.  The defining property: with the option on, every output of a call (final targets, start /
 * stop, gcount, ucount, seen bits, hits and their offsets, n_kmers, support records, tallies) is what the same call returns
 * with the option off on a text whose masked sequence bytes were replaced by 'N'.  start / stop do not change (trimming
 * reads the quality line alone), pos stays counted from the first byte of the read, n_kmers shrinks, and the support
 * rule's n is that smaller n_kmers.
 * One streaming kernel overwrites the masked bytes in the library's DEVICE copy of the text, in front of the kernels
 * that read it; the caller's text is never modified.  Because it writes in place, the FASTQ forms refuse, while an
 * option is > 0, a block whose lines are not in ascending order without overlap (KID_ERR_ARG): seq_off + seq_len <=
 * qual_off and qual_off + qual_len <= the next record's seq_off, as every indexer of a real file leaves them.
 *   KID_OPT_MIN_BASE_QUALITY     the sample's option, above: kid_classify_fastq_async (the mask kernel runs on the stream
 *                                of the prepare kernel, behind the upload of the block and in front of its classify kernels)
 *   KID_DB_OPT_MIN_BASE_QUALITY  the database's: kid_db_read_hits_fastq, _support_fastq and _segments_fastq, whose staged text is
 *                                masked in front of the hit pass (outside the interval kid_db_read_hits_time reports).  It
 *                                obeys the one-call-at-a-time rule of a kid_db and is NOT copied by kid_db_replicate.
 * The offsets and device forms of those calls have no quality text and are unaffected: mask their text first with the
 * two calls below.                                                                                                  */
#define KID_DB_OPT_MIN_BASE_QUALITY 1
int kid_db_set_option(kid_db *db, int option, int value);
/* bases masked in the sample's FASTQ blocks since kid_sample_begin / kid_sample_reset (synchronises).  Records with
 * qual_len < seq_len are not masked and not counted.  kid_sample_stats keeps its four fields.                       */
int kid_sample_masked_bases(kid_sample *s, uint64_t *out);
/* The companion of kid_trim_batch, host buffers: quals laid out like bases.  out_bases (laid out like bases, may equal
 * bases) receives the text of the reads with the masked bases replaced by 'N'; *n_masked (nullable) their number.
 * min_base_quality = 0 copies the text and reports 0; outside 0..93: KID_ERR_ARG.                                   */
int kid_mask_batch(kid_db *db, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads,
                   int min_base_quality, uint8_t *out_bases, uint64_t *n_masked);
/* In place on text resident in HBM, asynchronous on `stream`: use it in front of kid_classify_batch_device /
 * kid_db_read_hits_device on the same stream.  d_offsets: uint64[n_reads + 1], reads back to back (the bytes
 * offsets[0] .. offsets[n_reads] of d_bases are masked by the same bytes of d_quals); no alignment is asked of either.
 * d_n_masked: nullable; one uint64 that the number of bases masked is ADDED to (it is not reset).                    */
int kid_mask_batch_device(kid_db *db, void *d_bases, const void *d_quals, const void *d_offsets, uint64_t n_reads,
                          int min_base_quality, void *d_n_masked, void *stream);

/* ---- mask low-complexity sequence ----------------------------------------------------
 * A poly-A tail, a (CA)n microsatellite or a poly-G run is in every assembled genome and so in every database: one such
 * 30-mer calls a read, its qualities are fine, and a 40-base repeat gives 11 identical "supporting" hits.  With a
 * threshold T > 0 every base that lies in a low-complexity window is read as 'N' by everything behind the mask, in the
 * same way and under the same conditions as a low-quality base above (the device copy of the text, the caller's
 * untouched, a block's lines in ascending order without overlap while an option is on).
 * The rule -- a fixed-window, symmetric form of the DUST score, integers only:
 *   A line is one read's whole sequence s[0, len): the sequence line of a FASTQ record, [offsets[r], offsets[r+1]) in the
 *   offsets forms; the whole line, whatever its trimmed range.  Lines lying back to back never share a window.
 *   A byte is a base when the database's lookup takes it as one (ACGTacgt, Uu under KID_FLAG_U_IS_T).  Triplet i is valid
 *   when bytes i, i + 1, i + 2 are bases, and has the value 16 a + 4 b + c of their codes.
 *   The window of position p is [lo, hi) = [max(0, p - 32), min(len, p + 32)); l(p) is the number of valid triplets with
 *   lo <= i and i + 3 <= hi, c_v how many of them have value v, S(p) the sum of c_v (c_v - 1) / 2.
 *   p is low when l(p) >= 2 and 10 S(p) > T (l(p) - 1).  Every low position whose byte is a base becomes 'N'; nothing else
 *   is written.  All decisions of a line are taken on the text as it was before this mask wrote anything; where a
 *   quality option is on as well, the quality mask runs first and this rule sees its 'N's.
 * A call with the option on returns what the same call with the option off returns on the masked text: start / stop are
 * unchanged, pos is counted from the read's first byte, n_kmers is smaller (and is the n of the support rule).
 *   KID_OPT_LOW_COMPLEXITY     the sample's option, above: kid_classify_fastq_async (behind the quality mask, in front of
 *                              the prepare kernel, on the same stream)
 *   KID_DB_OPT_LOW_COMPLEXITY  the database's (kid_db_set_option; T in 0..1000, KID_ERR_ARG beyond): every FASTQ form of
 *                              kid_db_read_hits / _support / _segments / _fragments / _votes / _fragment_votes /
 *                              _segment_votes.  One call at a time, NOT copied by kid_db_replicate.
 * With both options off nothing is allocated or launched.                                                           */
#define KID_DB_OPT_LOW_COMPLEXITY 2
/* bases masked by KID_OPT_LOW_COMPLEXITY in the sample's FASTQ blocks since kid_sample_begin / kid_sample_reset
 * (synchronises); bases the quality mask took first are counted there, not here */
int kid_sample_lowc_bases(kid_sample *s, uint64_t *out);
/* Host buffers, per read: out_bases (laid out like bases, may equal bases) receives the text of the reads with the masked
 * bases replaced by 'N'; *n_masked (nullable) their number.  low_complexity = 0 copies the text and reports 0; outside
 * 0..1000: KID_ERR_ARG.  A record of any length: long ones are spread over many wavefronts.                        */
int kid_lowc_batch(kid_db *db, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int low_complexity,
                   uint8_t *out_bases, uint64_t *n_masked);
/* In place on text resident in HBM, asynchronous on `stream`, in front of kid_classify_batch_device /
 * kid_db_read_hits_device on the same stream.  d_offsets: uint64[n_reads + 1]; no alignment is asked of the text.
 * d_n_masked: nullable; one uint64 that the number of bases masked is ADDED to (it is not reset).  The host does not
 * see the lengths here: every read is one work item, which suits reads and not megabase records.                   */
int kid_lowc_batch_device(kid_db *db, void *d_bases, const void *d_offsets, uint64_t n_reads, int low_complexity,
                          void *d_n_masked, void *stream);

/* ---- every read's k-mer hits ------------------------------------------------------
 * What process_read folds (newkmer_10nx.cpp:526-595), handed out instead of folded: for every read, in read-position
 * order, the k-mer windows for which Hashtable::getHash returns a target > 0 (targets equal to 1 included).
 *   pos     index of the k-mer's first base, counted from the first byte of the read (not from `start`)
 *   target  what getHash returns
 *   entry   ordinal, in the arrays handed to kid_db_build, of the first-inserted entry with that key: the numbering
 *           of the seen-bitmap ("multi-GPU merge helpers" below), i.e. the line of the probes file
 * The calls are pure: they read the database and the caller's text and touch no sample (no gcount, no seen bit, no
 * stats).  Reads, ranges and trimming are decided by the kernels that decide them for kid_classify_*; the probe cap of
 * kmer_read_m3 (max_probes) is honoured.  Records of any length work.  The output is byte-identical across runs, across
 * any split of the reads into calls and across the table kinds (minimizer-localised, KID_FLAG_REF_GEOMETRY,
 * KID_FLAG_HOST_BUILD).
 *   hit_offsets[n_reads + 1]  CSR: the hits of read r are hits[hit_offsets[r] .. hit_offsets[r + 1]); always complete
 *   n_kmers[n_reads]          nullable; windows looked up per read (the read's share of kid_sample_stats' lookups)
 *   hits[cap], *n_hits        *n_hits = hit_offsets[n_reads], always; hits is filled only if *n_hits <= cap, otherwise
 *                             nothing is written to it and the call still returns KID_OK: size a buffer and call again
 *                             (hits = NULL, cap = 0 is the sizing call)
 * Argument errors as for kid_classify_batch (offsets not monotone, start/stop outside the read, more than 2^31-1
 * reads: KID_ERR_ARG; a quality line shorter than its sequence: KID_ERR_FORMAT).
 * Scratch: grows with the largest batch seen (16 B per read + 8 B per read for the tile index + 16 B per 64 windows,
 * plus, for the host-buffer forms, a device copy of the inputs and outputs), never with the database; it belongs to
 * the kid_db and is released by kid_db_destroy.  There is ONE set of it per kid_db, so calls on one kid_db run one after
 * the other: every call, the device form included, first blocks the calling thread until the kernels of the call before
 * are through.                                                                                                    */
typedef struct kid_hit {
    uint32_t pos, target, entry;
} kid_hit;
/* host buffers; offsets/start/stop as for kid_classify_batch (start = stop = NULL: whole reads) */
int kid_db_read_hits(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                     uint64_t n_reads, uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits);
/* a FASTQ text block as for kid_classify_fastq_async: process_qual runs on the GPU; a record that fails
 * stop - start >= k has n_kmers 0 and no hits */
int kid_db_read_hits_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                           uint64_t *hit_offsets, uint32_t *n_kmers, kid_hit *hits, uint64_t cap, uint64_t *n_hits);
/* Everything resident in HBM; the call returns once its kernels are queued on `stream` (but see above: it first waits
 * on the host for the call before it on this kid_db).  The alignment / lifetime rules of kid_classify_batch_device
 * hold for d_bases, d_offsets, d_start, d_stop.  d_hit_offsets: uint64[n_reads + 1]; d_n_kmers: uint32[n_reads], nullable;
 * d_hits: kid_hit[cap], nullable with cap = 0; d_n_hits: one uint64, written on the device.  What the host cannot
 * check is checked on the device and reported as KID_ERR_ARG by the next kid_db_read_hits_time: a [start, stop]
 * outside its read (clamped to the read), and a batch with more than bases_nbytes / 64 + n_reads tiles of 64 windows
 * (reads that overlap in the text, or offsets beyond bases_nbytes), which gets no hits at all: all offsets 0.      */
int kid_db_read_hits_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                            const void *d_stop, uint64_t n_reads, void *d_hit_offsets, void *d_n_kmers, void *d_hits, uint64_t cap,
                            void *d_n_hits, void *stream);
/* Device time of the hits kernels since the last query, the calls and the reads they belong to: one HIP event in front
 * of a call's first kernel (descriptors), one behind its last (fill).  For kid_db_read_hits_device that is the kernels
 * alone; the host-buffer forms read the number of hits back between count and fill (and may allocate), and that
 * round trip lies inside the interval.  Synchronises with the last call.                                           */
int kid_db_read_hits_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- calling reads by k-mer support -------------------------------------------------
 * kid_classify_* gives a read the target its hits fold to: one database k-mer among 121 windows calls a read.  These
 * calls ask for more evidence.  For one read let t_1 .. t_m be the targets of its hits in read-position order (exactly
 * the hits kid_db_read_hits reports, targets equal to 1 included) and n its n_kmers, the windows looked up.
 *   final      process_read's left fold of t_1 .. t_m with msca, 0 when m = 0: what kid_classify_* returns for the read
 *   S(c)       the number of hits whose target is c or a descendant of c; S(1) = m
 *   the rule   two integers, min_hits >= 0 and min_permille in 0..1000 (KID_ERR_ARG beyond)
 *   c passes   when S(c) >= min_hits and 1000 * S(c) >= min_permille * n   (64-bit integers; no floating point anywhere)
 *   confident  0 if final = 0; else the first node on the path final, parent(final), .., 1 that passes, 0 if none does.
 *              Under the rule (0, 0) confident = final for every read.
 * msca returns the deeper node of a lineage, so final need not be an ancestor of every hit: hits at targets [6, 8] with
 * 6 -> 8 fold to 8, with S(8) = 1 and S(6) = 2 -- which is what makes the climb meaningful.
 * One kernel turns the hits of a batch into one record per read; it is a pure function of the hits (no atomics): the
 * records are byte-identical across runs, splits of the batch into calls and table kinds.                            */
typedef struct kid_support {
    uint32_t final, confident, n_kmers, n_hits /* m */, s_final /* S(final), 0 if final = 0 */,
        s_confident /* S(confident), 0 if confident = 0 */;
} kid_support;
/* Host buffers, as kid_db_read_hits / kid_db_read_hits_fastq: the hit pass runs into scratch the kid_db owns (it grows
 * with the largest batch and its number of hits), then the support kernel; 24 bytes per read come back.  Errors as for
 * kid_db_read_hits*; the calls obey its one-call-at-a-time rule (one set of scratch per kid_db).
 *   out[n_reads]  nullable
 *   tally         nullable: a sample OF THIS kid_db (another's: KID_ERR_ARG) that is counted as if the batch had been
 *                 classified under the rule: gcount[confident]++ for exactly the reads kid_classify_batch /
 *                 kid_classify_fastq_async would count (a read shorter than k handed in with whole-read ranges under
 *                 target 0; a FASTQ record that fails stop - start >= k nowhere), and, for reads with confident > 0, the
 *                 seen bit of every hit with target > 1.  The tally kernel runs in the sample's stream, behind whatever
 *                 the sample has queued.  Classifying and tallying into one sample may be mixed; kid_sample_end,
 *                 kid_sample_end_merged, kid_sample_reset and the seen-bitmap helpers work on a tallied sample as on any
 *                 other.  kid_sample_stats is NOT updated by a tally.  A tally after kid_sample_end / _end_merged
 *                 without kid_sample_reset is KID_ERR_STATE.  A batch the hit pass refuses is not counted at all.     */
int kid_db_read_support(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                        uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally);
int kid_db_read_support_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                              uint32_t min_hits, uint32_t min_permille, kid_support *out, kid_sample *tally);
/* The kernel alone, for a CSR that is in HBM already (kid_db_read_hits_device with a d_hits that held all the hits):
 * d_hit_offsets uint64[n_reads + 1], d_hits kid_hit[] (may be NULL when there is no hit), d_n_kmers uint32[n_reads],
 * d_out kid_support[n_reads].  Asynchronous on `stream`; the host need not know the number of hits; no tally.  Like
 * every call on a kid_db it first waits on the host for the kernels of the call before it.  A target outside
 * (0, ntar) in d_hits is read as the root.                                                                          */
int kid_db_support_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                    uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream);
/* Device time of the support kernel ALONE since the last query (HIP events around it), its calls and reads; the hit pass
 * of the host forms is in kid_db_read_hits_time.  Synchronises with the last call.                                  */
int kid_db_read_support_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- one call per fragment ------------------------------------------------------------
 * kid_db_read_support* judges every read on its own.  Two reads that are mates of one sequenced fragment are one piece
 * of evidence: these calls call the pair as one unit.  A fragment is an ordered pair of reads, mate 1 and mate 2.
 * Either may be absent, or may have no window.
 *   hits       Let a_1 .. a_p be the hits of mate 1 and b_1 .. b_q those of mate 2.  They are exactly what
 *              kid_db_read_hits reports for each mate: the same pos, target and entry, in read-position order, targets
 *              equal to 1 included.  They are taken under the mate's own trimmed range.  n_1 and n_2 are the mates'
 *              n_kmers.
 *   sequence   The fragment's hit sequence is a_1 .. a_p, b_1 .. b_q: mate 1 first.  Let m = p + q and n = n_1 + n_2.
 *              No window spans the two mates.  Nothing is reverse-complemented beyond what the lookup already does per
 *              k-mer.
 *   six fields final, confident, n_kmers, n_hits, s_final and s_confident are exactly the kid_support record above,
 *              applied to that sequence with that n, under (min_hits, min_permille).
 *   per mate   final_1 is the left fold of a_1 .. a_p alone, and final_2 that of b_1 .. b_q alone.  Each is 0 without a
 *              hit.  These are what kid_classify_* returns for each mate.
 * msca is not associative, so final is NOT msca(final_1, final_2) in general.  Take mate 1 = [8] and mate 2 = [X, 6],
 * with 6 an ancestor of 8 and X outside that lineage.  The pair folds 8 -> 1 -> 6, while msca(8, msca(X, 6)) =
 * msca(8, 1) = 8.  The fold is one left fold over m hits that continues from final_1 into mate 2's hits.
 * One kernel turns the hits of a batch into one record per fragment; it is a pure function of the hits (no atomics): the
 * records are byte-identical across runs and splits of the batch into calls.                                          */
typedef struct kid_fragment {
    uint32_t final, confident, n_kmers /* n */, n_hits /* m */, s_final, s_confident, final_1, final_2;
} kid_fragment;
/* Host buffers, as kid_db_read_support.  The batch holds n_reads = 2 F reads in interleaved order: read 2i is mate 1 of
 * fragment i, and read 2i + 1 is its mate 2 (an absent mate is an empty read).  n_reads odd is KID_ERR_ARG;
 * min_permille > 1000 and null pointers are KID_ERR_ARG; n_reads = 0 returns KID_OK and launches nothing.
 *   out[n_reads / 2]  nullable with a tally
 *   tally             nullable: a sample OF THIS kid_db (another's: KID_ERR_ARG; one that has ended: KID_ERR_STATE).  A
 *                     counted fragment adds 1 to gcount[confident]: once per fragment, under 0 when confident = 0.
 *                     When confident > 0, the fragment sets the seen bit of every hit of BOTH mates with target > 1.
 *                     Under KID_OPT_ENTRY_DEPTH, the same fragment adds 1 to depth[entry] per such hit; a k-mer present
 *                     in both mates adds 2.  In the offsets and device forms every fragment is counted.  In the FASTQ
 *                     form a fragment is counted when at least one of its mates is kept by process_qual; a dropped mate
 *                     contributes no hit and no window, and a fragment with both mates dropped is counted nowhere.
 *                     kid_sample_stats is NOT updated.  A batch the hit pass refuses is not counted at all.           */
int kid_db_read_fragments(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                          uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment *out, kid_sample *tally);
/* Two blocks of FASTQ text with their line indexes: record i of recs1 is mate 1 of fragment i and record i of recs2 its
 * mate 2.  Either recs pointer may point into the middle of a block's record index.  A record with seq_len = 0 and
 * qual_len = 0 is an absent mate.  The blocks are staged as one text with one interleaved index: nbytes1 + nbytes2 must
 * stay below 4 GiB (KID_ERR_ARG).  KID_DB_OPT_MIN_BASE_QUALITY applies as in kid_db_read_support_fastq; its "lines
 * ascending, no overlap" check runs per block.  A quality line shorter than its sequence in either block is
 * KID_ERR_FORMAT.                                                                                                    */
int kid_db_read_fragments_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t min_hits,
                                uint32_t min_permille, kid_fragment *out, kid_sample *tally);
/* The kernel alone on an interleaved CSR in HBM (the companion of kid_db_support_from_hits_device, same arguments):
 * d_hit_offsets uint64[n_reads + 1], d_n_kmers uint32[n_reads], d_out kid_fragment[n_reads / 2].  Asynchronous on
 * `stream`; no tally.  A target outside (0, ntar) in d_hits is read as the root.                                     */
int kid_db_fragments_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                      uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream);
/* Device time of the fragment kernel ALONE since the last query, its calls and fragments.  Synchronises with the last
 * call.                                                                                                              */
int kid_db_read_fragments_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments);

/* ---- calling reads by root-path votes ----------------------------------------------------
 * `final` is a left fold with msca, which is neither associative nor symmetric: the lookup is canonical, so a read and
 * its reverse complement have the same hits in opposite order and can fold to different targets (hits [X, 8, 6] with
 * 6 -> 8 and X on another lineage fold to 6, [6, 8, X] to 1).  These calls weigh the hits on the tree instead; the
 * record is a pure function of the MULTISET of the read's hit targets and its n_kmers.  With t_1 .. t_m and n as for
 * kid_db_read_support (the hits of kid_db_read_hits, targets equal to 1 included):
 *   w(c)       the number of hits with t_i = c
 *   P(c)       the number of hits whose target is c or an ancestor of c: the sum of w over c's root path.  A hit at the
 *              root counts for every node.
 *   best       the largest P(t_i); L = the distinct hit targets with P = best.  P strictly grows down a lineage of hit
 *              nodes, so no two members of L lie on one lineage.
 *   call       the lowest common ancestor of L: the deepest node that is on every member's root path (NOT msca).  With
 *              one member it is that target; 0 when m = 0.
 *   S(c), the rule and "c passes" are those of kid_db_read_support.
 *   confident  the first node on call, parent(call), .., 1 that passes, 0 if none does or call = 0.  Under the rule
 *              (0, 0) confident = call for every read.
 * On the tree 5 -> 6 -> 8, 5 -> 35 -> 36: [6, 8] -> call 8, p_best 2; [X, 8, 6] -> 8; [8, 36] -> a tie, call 5,
 * n_best 2; [X, 8] -> a tie, call 1; [1, X] -> call X, p_best 2; [8, 8, 36, 36, X] -> call 5 (its fold ends at 1).
 * The records are byte-identical across runs, splits of the batch into calls, table kinds and any permutation of a
 * read's hits.  Reads of more than a few hundred hits are settled by a second kernel queued behind the first.       */
typedef struct kid_vote {
    uint32_t call, confident, n_kmers, n_hits /* m */, p_best /* best, 0 without a hit */, n_best /* |L| */,
        s_call /* S(call), 0 if call = 0 */, s_confident /* S(confident), 0 if confident = 0 */;
} kid_vote;
/* The four forms of kid_db_read_support*, argument for argument: host buffers (32 bytes per read come back), a FASTQ
 * block (KID_DB_OPT_MIN_BASE_QUALITY applies as in kid_db_read_support_fastq), the kernels alone on a CSR in HBM
 * (asynchronous on `stream`, no tally; a target outside (0, ntar) is read as the root), and the device time of the vote
 * kernels ALONE since the last query.  Errors and the one-call-at-a-time rule are theirs: min_permille > 1000 is
 * KID_ERR_ARG, n_reads = 0 returns KID_OK and launches nothing.
 *   tally      as in kid_db_read_support with `confident` as defined here: gcount[confident]++ per counted read; for
 *              reads with confident > 0 the seen bit of every hit with target > 1, and depth[entry] under
 *              KID_OPT_ENTRY_DEPTH.  A sample of another kid_db is KID_ERR_ARG, one that has ended KID_ERR_STATE.
 * Scratch beside the hit pass's: 4 bytes per read of the largest batch and one row of 4 * ntar bytes per compute unit,
 * owned by the kid_db and released by kid_db_destroy.                                                               */
int kid_db_read_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                      uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally);
int kid_db_read_votes_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                            uint32_t min_hits, uint32_t min_permille, kid_vote *out, kid_sample *tally);
int kid_db_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                  uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream);
int kid_db_read_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- calling fragments by root-path votes -------------------------------------------------
 * kid_db_read_fragments* calls a pair as one unit but by the left fold, so the call can change when the mates are
 * exchanged; kid_db_read_votes* is independent of hit order but judges every mate on its own.  These calls vote over the
 * fragment.  The batch holds 2 F reads interleaved as for kid_db_read_fragments.  With a_1 .. a_p, b_1 .. b_q the hits
 * of the two mates as kid_db_read_hits reports them and n_1, n_2 their n_kmers:
 *   multiset     The fragment's hit multiset is {a_1 .. a_p} + {b_1 .. b_q}, with m = p + q.  n = n_1 + n_2 is computed
 *                in uint32 exactly as kid_fragment.n_kmers is.  An absent or empty mate contributes nothing.
 *   eight fields call, confident, n_kmers, n_hits, p_best, n_best, s_call and s_confident are exactly the kid_vote record
 *                above of a read with those m hits and that n, under (min_hits, min_permille).  A target outside
 *                (0, ntar) is read as the root.
 *   per mate     call_1 is the vote call of a_1 .. a_p alone and call_2 that of b_1 .. b_q alone.  Each is 0 without a
 *                hit.  They are what kid_db_read_votes returns as `call` for reads 2i and 2i + 1.
 * The record is invariant under any permutation of the hits inside each mate; exchanging the two mates exchanges call_1
 * and call_2 and changes nothing else; with q = 0 the first eight fields are mate 1's kid_vote record except that
 * n_kmers = n_1 + n_2; when all m hits lie on one root path, call = kid_fragment.final.
 * On the tree 5 -> 6 -> 8, 5 -> 35 -> 36, X on another lineage (mate 1 | mate 2 -> call, p_best, n_best, call_1, call_2):
 *   [8] | [36] -> 5, 1, 2, 8, 36        [X, 8] | [6] -> 8, 2, 1, 1, 6 (mate 1 alone is a tie)
 *   [8] | [X, 6] -> 8, 2, 1, 8, 1 (kid_fragment.final is 6 here)        [] | [6, 8] -> 8, 2, 1, 0, 8
 * Fragments of more than a few hundred hits in total are settled by a second kernel queued behind the first.         */
typedef struct kid_fragment_vote {
    uint32_t call, confident, n_kmers /* n */, n_hits /* m */, p_best, n_best, s_call, s_confident, call_1, call_2;
} kid_fragment_vote;
/* The four forms of kid_db_read_fragments*, argument for argument: host buffers (n_reads = 2 F; 40 bytes per fragment
 * come back), two FASTQ blocks (nbytes1 + nbytes2 below 4 GiB, at most 2^30 - 1 fragments; KID_DB_OPT_MIN_BASE_QUALITY
 * and KID_DB_OPT_LOW_COMPLEXITY apply as in kid_db_read_fragments_fastq), the kernels alone on an interleaved CSR in
 * HBM (d_out kid_fragment_vote[n_reads / 2]; asynchronous on `stream`, no tally), and the device time of the
 * fragment-vote kernels ALONE since the last query.  The error statuses are those of kid_db_read_fragments*, in the same
 * order: n_reads odd, min_permille > 1000 and null pointers are KID_ERR_ARG; n_reads = 0 returns KID_OK.
 *   tally      exactly as in kid_db_read_fragments with `confident` as defined here: gcount[confident]++ once per
 *              counted fragment, under 0 when confident = 0; for fragments with confident > 0 the seen bit of every hit
 *              of both mates with target > 1, and depth[entry]++ per such hit under KID_OPT_ENTRY_DEPTH.  The FASTQ
 *              form counts a fragment when at least one mate is kept by process_qual.  kid_sample_stats is NOT updated.
 * Scratch of its own beside the vote calls': 4 bytes per fragment of the largest batch and one row of 4 * ntar bytes per
 * compute unit, owned by the kid_db and released by kid_db_destroy.                                                  */
int kid_db_read_fragment_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                               uint64_t n_reads, uint32_t min_hits, uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally);
int kid_db_read_fragment_votes_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                     uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t min_hits,
                                     uint32_t min_permille, kid_fragment_vote *out, kid_sample *tally);
int kid_db_fragment_votes_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                           uint32_t min_hits, uint32_t min_permille, void *d_out, void *stream);
int kid_db_read_fragment_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments);

/* ---- calling records in segments ------------------------------------------------------
 * kid_db_read_support* gives a record one answer.  A contig that is one species for its first 1.4 Mb and another after
 * that, a chimeric long read or a transferred island folds to an ancestor and nothing says where the change is.  These
 * calls cut every record into segments and call each segment by its own hits under the same rule.
 * "Window" keeps its meaning (one k-mer position of a read).  For one read with the trimmed range [start, stop]:
 *   P          = max(0, stop - start + 1 - (k - 1)) window positions (0 as well for a FASTQ record process_qual drops);
 *                position q in 0..P-1 is the window whose first base is byte start + q of the read
 *   seg_len    >= 1, in window positions; seg_step in 1..seg_len; seg_len <= 1024 * seg_step
 *              (KID_SEGMENT_MAX_OVERLAP: a position lies in at most 1024 segments); anything else is KID_ERR_ARG
 *   n_seg      0 if P = 0; 1 if P <= seg_len; otherwise 1 + ceil((P - seg_len) / seg_step)
 *   segment j  covers the positions [j * seg_step, min(j * seg_step + seg_len, P)): every position is covered, only the
 *              last segment may be shorter than seg_len, it ends at P, and no segment lies inside the one before it
 * The record of a segment:
 *   pos        start + j * seg_step: counted from the first byte of the read, as kid_hit.pos is
 *   n_pos      the positions it covers
 *   the rest   the kid_support record kid_db_read_support returns under the same (min_hits, min_permille) for that read
 *              with the range [pos, pos + n_pos + k - 2]: n_kmers counts the covered positions whose window holds a
 *              k-mer and is the n of the permille test; the hits are those of kid_db_read_hits with pos in
 *              [pos, pos + n_pos), folded in position order
 * With seg_len >= every read's P each read with P > 0 has exactly one segment: its kid_support record, pos = start,
 * n_pos = P.  The segment list is dense: segments without a hit are there, with final = confident = 0.
 *   seg_offsets[n_reads + 1]   CSR: the segments of read r are segments[seg_offsets[r] .. seg_offsets[r + 1]); always complete
 *   segments[cap], *n_segments *n_segments = seg_offsets[n_reads], always; segments is filled only if *n_segments <= cap,
 *                              otherwise nothing is written to it and the call still returns KID_OK (segments = NULL,
 *                              cap = 0 is the sizing call): the convention of kid_db_read_hits
 * The calls are pure (no sample, no tally, no atomics); the output is byte-identical across runs, across any split of the
 * reads into calls and across the table kinds.  A segment's numbers come from two prefix arrays over the tiles of the hit
 * pass and cost the same whatever its length; its hits are folded by kid_db_read_support's code.
 * Errors as for kid_db_read_hits*, plus the parameter errors above and min_permille > 1000 (KID_ERR_ARG).  The calls obey
 * the one-call-at-a-time rule of a kid_db's scratch, to which they add 16 B per tile of 64 windows (valid mask and its
 * scan), 8 B per read (first segment) and 32 B per segment (host forms); it is released by kid_db_destroy.            */
#define KID_SEGMENT_MAX_OVERLAP 1024u
typedef struct kid_segment {
    uint32_t pos, n_pos, final, confident, n_kmers, n_hits, s_final, s_confident;
} kid_segment;
/* host buffers; offsets/start/stop as for kid_db_read_hits */
int kid_db_read_segments(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                         uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                         uint64_t *seg_offsets, kid_segment *segments, uint64_t cap, uint64_t *n_segments);
/* a FASTQ text block as for kid_db_read_hits_fastq (KID_DB_OPT_MIN_BASE_QUALITY is honoured the same way); a dropped
 * record has no segment */
int kid_db_read_segments_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                               uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille, uint64_t *seg_offsets,
                               kid_segment *segments, uint64_t cap, uint64_t *n_segments);
/* Everything resident in HBM, asynchronous on `stream`; inputs as for kid_db_read_hits_device.  d_hits / hits_cap: the
 * caller's scratch for the hits (kid_hit[hits_cap]); d_seg_offsets: uint64[n_reads + 1]; d_segments: kid_segment[seg_cap];
 * d_n_hits, d_n_segments: one uint64 each, written on the device.  If the hits exceed hits_cap or the segments seg_cap
 * no segment is written; both counts and d_seg_offsets are still complete.  What the host cannot check is reported by
 * the next kid_db_read_hits_time, as for kid_db_read_hits_device (such a batch has no segment).                     */
int kid_db_read_segments_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                const void *d_stop, uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits,
                                uint32_t min_permille, void *d_hits, uint64_t hits_cap, void *d_seg_offsets, void *d_segments,
                                uint64_t seg_cap, void *d_n_hits, void *d_n_segments, void *stream);
/* Device time of the segment kernels ALONE since the last query (the two scans and the segments kernel; the host forms
 * read the number of segments back in between), their calls and reads; the hit pass is in kid_db_read_hits_time.     */
int kid_db_read_segments_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- calling segments by root-path votes ------------------------------------------------
 * kid_db_read_segments* calls every segment by the left fold, which depends on the order of the hits: a record and its
 * reverse complement carry the same hits in opposite order, so a contig assembled on the other strand can get other
 * segment calls.  These calls cut the record exactly as kid_db_read_segments* does -- seg_len, seg_step and their limits,
 * P, n_seg, the coverage of segment j, pos and n_pos are those above, and the list is dense -- and call each segment by the
 * vote rule of kid_db_read_votes*.  The record of a segment:
 *   pos, n_pos   those of kid_segment
 *   the rest     the kid_vote record kid_db_read_votes returns under the same (min_hits, min_permille) for that read with
 *                the range [pos, pos + n_pos + k - 2]: the vote record over the multiset of targets of the read's hits
 *                with pos in [pos, pos + n_pos), n = the covered positions whose window holds a k-mer.  A target outside
 *                (0, ntar) is read as the root.  A segment without a hit has call = confident = p_best = n_best =
 *                s_call = s_confident = 0.
 * seg_offsets, pos, n_pos, n_kmers and n_hits equal those of kid_db_read_segments for the same arguments.  With seg_len >=
 * every read's P each read with P > 0 has one segment, whose eight vote fields are its kid_vote record.  When all hits of
 * a segment lie on one root path, call = kid_segment.final.  For a record with P <= seg_len or (P - seg_len) % seg_step
 * == 0, segment j of the record is segment n_seg - 1 - j of its reverse complement in n_pos and all eight vote fields.
 * The calls are pure (no sample, no tally, no atomics on outputs); the output is byte-identical across runs, across any
 * split of the reads into calls and across the table kinds.  A segment of more than a few hundred hits is settled by a
 * second kernel queued behind the first; under overlap every hit is visited once per segment that covers it.
 * The four forms mirror kid_db_read_segments* argument for argument, with the same error statuses in the same order, the
 * same sizing call (segments = NULL, cap = 0), the same handling of n_reads = 0 and of hits_cap / seg_cap (nothing is
 * written to d_segments when either is exceeded; the counts and d_seg_offsets are still complete).
 * KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY apply to the FASTQ form as they do to
 * kid_db_read_segments_fastq.  Scratch beside that of kid_db_read_segments*: 40 B per segment (host forms), 24 B per
 * segment the call can write (the list for the second kernel: the host forms' total, the device form's seg_cap) and the
 * rows of kid_db_read_votes*.  _time: the device time of the two scans and the two segment-vote kernels ALONE since the
 * last query, their calls and reads.                                                                                   */
typedef struct kid_segment_vote {
    uint32_t pos, n_pos, call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident;
} kid_segment_vote;
int kid_db_read_segment_votes(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                              uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille,
                              uint64_t *seg_offsets, kid_segment_vote *segments, uint64_t cap, uint64_t *n_segments);
int kid_db_read_segment_votes_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                                    uint32_t seg_len, uint32_t seg_step, uint32_t min_hits, uint32_t min_permille, uint64_t *seg_offsets,
                                    kid_segment_vote *segments, uint64_t cap, uint64_t *n_segments);
int kid_db_read_segment_votes_device(kid_db *db, const void *d_bases, uint64_t bases_nbytes, const void *d_offsets, const void *d_start,
                                     const void *d_stop, uint64_t n_reads, uint32_t seg_len, uint32_t seg_step, uint32_t min_hits,
                                     uint32_t min_permille, void *d_hits, uint64_t hits_cap, void *d_seg_offsets, void *d_segments,
                                     uint64_t seg_cap, void *d_n_hits, void *d_n_segments, void *stream);
int kid_db_read_segment_votes_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- placing reads on a genome by colinear hits --------------------------------------------
 * Every call above uses a hit's target alone.  A hit also says where on which genome its probe lies: a line of the
 * probes file is SEQ,target,org,position,strand,count.  The hits of a read that is a stretch of genome g lie on one
 * diagonal -- position - pos is the same for all of them when the read is forward, position + pos when it is reverse --
 * and spurious hits, hits in repeats and the two halves of a chimeric read do not.  These calls find, per read, the
 * diagonal most hits agree on.  Integers only; targets play no role.
 * Sites: two host arrays uint32[n_entries] in the numbering of kid_hit.entry (what load_probes_gz(.., want_sites) and
 * read_probe_sites yield): org[o] < 2^24 = KID_LOCI_MAX_ORGS and pos[o] < 2^31, n_entries the database's own; anything
 * else is KID_ERR_ARG and changes nothing.  org = pos = NULL with n_entries = 0 frees the sites; a second call replaces
 * them.  8 bytes of HBM per entry, owned by the kid_db; NOT copied by kid_db_replicate.  Synchronises the device.       */
#define KID_LOCI_MAX_ORGS (1u << 24)
#define KID_LOCI_MAX_HITS 4096u
int kid_db_set_sites(kid_db *db, const uint32_t *org, const uint32_t *pos, uint64_t n_entries);
/* For one read let h_1 .. h_m be its hits as kid_db_read_hits reports them, n its n_kmers and W >= 1 the diagonal bin
 * width diag_bin.
 *   participants  the first min(m, KID_LOCI_MAX_HITS) hits in list order; of these a hit with entry >= n_entries (possible
 *                 in the from-hits form alone) is ignored: it counts in n_hits and nowhere else.  Hits with target 1 or
 *                 a target outside (0, ntar) take part like any other.
 *   keys          participant i with g = org[entry_i], x = pos[entry_i], r = pos_i has the forward key
 *                 (g, 0, floor((x - r) / W)) and the reverse key (g, 1, (x + r) / W): 64-bit signed arithmetic, floor
 *                 toward minus infinity.  c(key) is the number of participants that have the key.
 *   best key      the largest c; ties go to strand 0 before strand 1, then the lowest g, then the lowest diagonal.  The
 *                 chain is the set of participants with the best key.
 *   org, strand   those of the best key;  n_chain its c
 *   n_org         the participants with g = org, on whatever diagonal
 *   n_other       the largest c(key) over keys with g != org, 0 when there is none: the evidence for a chimera
 *   n_hits        m: all hits, those beyond KID_LOCI_MAX_HITS and the ignored ones included;  n_kmers = n
 *   pos_first, pos_last  the smallest and largest pos in the chain
 *   entry_first   the entry of the chain hit at pos_first (the lowest if several share that pos): the chain lies at genome
 *                 coordinate pos[entry_first] at read position pos_first
 * Without a participant every field but n_hits and n_kmers is 0; n_chain = 0 says so.  With one, n_chain = 1 and strand = 0
 * by the tie order: the strand then carries no information.
 * For m <= KID_LOCI_MAX_HITS the record is a pure function of the multiset of (pos, entry) and of n: the same under any
 * permutation of the hits, byte-identical across runs, splits of a batch into calls and table kinds.  No atomics on
 * outputs; reads of more than a few hundred hits are settled by a second kernel queued behind the first.
 * There is no rule, no tally and no sample: a locus is not a count.                                                   */
typedef struct kid_locus {
    uint32_t org, strand, n_chain, n_org, n_other, n_hits /* m */, n_kmers, pos_first, pos_last, entry_first;
} kid_locus;
/* The forms of kid_db_read_support* with diag_bin in the place of the rule and without a tally: host buffers (40 bytes per
 * read come back), a FASTQ block (KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY apply as in
 * kid_db_read_hits_fastq), the kernels alone on a CSR in HBM (d_out: kid_locus[n_reads]; asynchronous on `stream`), and the
 * device time of the loci kernels ALONE since the last query.  Errors and the one-call-at-a-time rule are theirs, in the
 * same order, with diag_bin = 0 KID_ERR_ARG where they refuse a rule, and a database without sites KID_ERR_STATE (nothing
 * is allocated or launched) behind the check of n_reads; out = NULL with reads is KID_ERR_ARG; n_reads = 0 returns KID_OK
 * and launches nothing.  Scratch beside the hit pass's: 4 bytes per read of the largest batch.                        */
int kid_db_read_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                     uint64_t n_reads, uint32_t diag_bin, kid_locus *out);
int kid_db_read_loci_fastq(kid_db *db, const uint8_t *text, uint64_t text_nbytes, const kid_fastq_rec *recs, uint64_t n_reads,
                           uint32_t diag_bin, kid_locus *out);
int kid_db_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                 uint32_t diag_bin, void *d_out, void *stream);
int kid_db_read_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *reads);

/* ---- placing mate pairs as one fragment by colinear hits ------------------------------------
 * The two mates of a pair are the two ends of one fragment: on the same genome, on opposite strands, a few hundred bases
 * apart.  One hit in each mate that agree on this is a chain of two, with a strand, an insert size and a genome interval
 * that includes the unsequenced middle -- where kid_db_read_loci gives each mate n_chain = 1 and a strand that says nothing.
 * The choice is joint: it cannot be made from the two mates' kid_locus records.  Integers only; targets play no role; no
 * rule, no tally, no sample.
 * The batch holds 2 F reads interleaved as for kid_db_read_fragments; an absent or empty mate contributes nothing.  W =
 * diag_bin >= 1, max_span >= 0 in bases, k the database's k-mer length.
 *   participants  per mate s, exactly those of kid_db_read_loci for that read: the first min(m_s, KID_LOCI_MAX_HITS) hits
 *                 in list order whose entry < n_entries
 *   keys          per mate, exactly kid_db_read_loci's: forward (g, floor((x - r) / W)), reverse (g, (x + r) / W).  F_s(g, D)
 *                 is the number of participants of mate s with the forward key (g, D), R_s(g, E) with the reverse key (g, E)
 *   paired placement (o, g, D, E)  o = 0 takes F_1(g, D) >= 1 and R_2(g, E) >= 1 (mate 1 forward, mate 2 reverse), o = 1
 *                 takes F_2(g, D) >= 1 and R_1(g, E) >= 1.  Allowed when D <= E and (E - D) * W <= max_span (64-bit).  Its
 *                 score is the sum of the two counts.  With W = 1, E - D is the insert length minus k
 *   solo placement (s, t, g, d)    one key of one mate, t = 0 forward or 1 reverse, its count the score; its orient is t for
 *                 s = 1 and 1 - t for s = 2: orient = 0 always means "mate 1 reads forward"
 *   best          the highest score; ties: a paired placement before a solo one; paired ones by (o, g, D, E) ascending;
 *                 solo ones by (t, g, d, s) ascending (with one mate absent: kid_db_read_loci's tie order)
 *   org, orient   those of the best placement;  mates  3 for a paired best, s for a solo best, 0 without a participant
 *   n_chain       the best score;  n_chain_s  the count of the chosen key within mate s, 0 for a mate that is not in the
 *                 placement: n_chain = n_chain_1 + n_chain_2
 *   n_org         the participants of both mates with org[entry] = org
 *   n_other       the largest score of any placement, paired or solo, with g != org; 0 when there is none
 *   n_hits        m_1 + m_2, all hits;  n_kmers = n_1 + n_2 in uint32, as kid_fragment.n_kmers
 *   pos_first_s, pos_last_s  the smallest and largest read position in mate s's chain (the participants of mate s that
 *                 have the chosen key); 0 for a mate that is not in the placement
 *   lo, hi        for each mate in the placement: a = pos[entry] of its chain hit at pos_first_s (the lowest entry if several
 *                 share that position), d = pos_last_s - pos_first_s; a forward key covers [a, a + d + k - 1], a reverse key
 *                 [max(0, a - d), a + k - 1] (the pileup's formula for a read).  lo is the smallest low end and hi the
 *                 largest high end over the mates in the placement; hi saturates at 2^32 - 1.  With W = 1 and a paired best
 *                 [lo, hi] is the fragment's genome interval as far as its k-mers show it
 * Without a participant every field but n_hits and n_kmers is 0.
 * Worked case.  k = 30, W = 1, max_span = 1000; entries 0..4 with the sites (org, pos) = (3,100) (3,130) (3,400) (9,40)
 *   (3,5000); mate 1 has the hits (pos, entry) = (10,0) (40,1) (5,3), mate 2 (60,2) (20,4).  Mate 1's forward keys on org 3
 *   are 90, 90; mate 2's reverse keys on org 3 are 460 and 5020.  (o = 0, g = 3, D = 90, E = 460) is allowed (370 <= 1000)
 *   and scores 3; no other pair is allowed.  The record: org 3, orient 0, mates 3, n_chain 3, n_chain_1 2, n_chain_2 1,
 *   n_org 4, n_other 1, n_hits 5, n_kmers 242, lo 100, hi 429, pos_first_1 10, pos_last_1 40, pos_first_2 60, pos_last_2 60.
 *   (The fragment starts at 90; mate 2 of 150 bases ends at 489: the insert is 400 = E - D + k.)  With the mates exchanged
 *   orient is 1 and the _1 / _2 fields swap.  Under max_span = 369 the pair is refused and the best is mate 1 alone: mates
 *   1, n_chain 2, lo 100, hi 159.  With one hit each, (10,0) and (60,2): mates 3, n_chain 2, orient 0, lo 100, hi 429.
 * While each mate has at most KID_LOCI_MAX_HITS hits the record is a pure function of the two multisets of (pos, entry) and
 * of n_1 + n_2: the same under any permutation of the hits inside a mate, byte-identical across runs, splits of a batch
 * into calls at even read indexes and table kinds.  With mate 2 without a participant, org, orient (= strand), n_chain,
 * n_org, n_other, pos_first_1 and pos_last_1 are mate 1's kid_locus and [lo, hi] is the interval the pileup gives it; the
 * mirror holds for mate 2 with strand = 1 - orient.  No atomics on outputs; a fragment with more than a few hits in either
 * mate is settled by a second kernel queued behind the first, whose worst case is one test per allowed pair of keys.     */
typedef struct kid_fragment_locus {
    uint32_t org, orient, mates, n_chain, n_chain_1, n_chain_2, n_org, n_other, n_hits /* m_1 + m_2 */, n_kmers, lo, hi, pos_first_1, pos_last_1,
        pos_first_2, pos_last_2;
} kid_fragment_locus;
/* The forms of kid_db_read_fragments* argument for argument, with (diag_bin, max_span) in the place of the rule and without
 * a tally: host buffers (64 bytes per fragment come back; out[n_reads / 2]), two FASTQ blocks (KID_DB_OPT_MIN_BASE_QUALITY
 * and KID_DB_OPT_LOW_COMPLEXITY apply as in kid_db_read_fragments_fastq), the kernels alone on an interleaved CSR in HBM
 * (d_out: kid_fragment_locus[n_reads / 2]; asynchronous on `stream`), and the device time of the fragment-loci kernels
 * ALONE since the last query.  Refused, in this order: what kid_db_read_fragments* refuses -- too many reads, n_reads odd,
 * out = NULL with reads: KID_ERR_ARG --, then diag_bin = 0 KID_ERR_ARG, then a database without sites KID_ERR_STATE
 * (nothing is allocated or launched); then n_reads = 0 returns KID_OK and launches nothing; then the batch's own null
 * pointers, KID_ERR_ARG.  The one-call-at-a-time rule of every call on a kid_db holds.  Scratch beside the hit pass's: 4
 * bytes per fragment of the largest batch.                                                                            */
int kid_db_read_fragment_loci(kid_db *db, const uint8_t *bases, const uint64_t *offsets, const int32_t *start, const int32_t *stop,
                              uint64_t n_reads, uint32_t diag_bin, uint32_t max_span, kid_fragment_locus *out);
int kid_db_read_fragment_loci_fastq(kid_db *db, const uint8_t *text1, uint64_t nbytes1, const kid_fastq_rec *recs1, const uint8_t *text2,
                                    uint64_t nbytes2, const kid_fastq_rec *recs2, uint64_t n_fragments, uint32_t diag_bin, uint32_t max_span,
                                    kid_fragment_locus *out);
int kid_db_fragment_loci_from_hits_device(kid_db *db, const void *d_hit_offsets, const void *d_hits, const void *d_n_kmers, uint64_t n_reads,
                                          uint32_t diag_bin, uint32_t max_span, void *d_out, void *stream);
int kid_db_read_fragment_loci_time(kid_db *db, double *device_ms, uint64_t *calls, uint64_t *fragments);

/* ---- placed reads piled up per genome bin ---------------------------------------------------
 * kid_locus records added up: how many placed reads cover each stretch of each genome.  Integers only.
 * Geometry.  A pileup belongs to one kid_db that has sites and to a bin width W >= 1; its geometry is that of
 *   kid_seen_coverage for the same W (see below), so the two profiles line up bin for bin:
 *   n_orgs = the largest org of the sites + 1;  span_bins[g] = 1 + max(pos[o] / W) over the entries of organism g, 0 when
 *   it has none;  bin_base = the exclusive scan of span_bins;  B = their sum.  B > KID_COVERAGE_MAX_BINS is KID_ERR_ARG,
 *   before anything of B elements is allocated.
 * Counters.  Two uint32 per bin, starts[g][b] and depth[g][b], zero after creation and after kid_pileup_reset; two uint64
 *   beside them, n_records (records handed in) and n_placed.  The per-bin counters are exact while a pileup has placed
 *   fewer than 2^32 records; beyond that they are taken modulo 2^32.
 * Placing.  One call adds a list of records under min_chain >= 1 and min_margin >= 0.  A record L is placed when
 *   L.n_chain >= min_chain,  (L.n_chain >= L.n_other ? L.n_chain - L.n_other : 0) >= min_margin,  L.strand <= 1,
 *   L.entry_first < n_entries  and  L.org == org[L.entry_first] (which implies span_bins[L.org] >= 1); otherwise it changes
 *   nothing.  Records kid_db_read_loci* produced with n_chain >= 1 always satisfy the last three; the device form may be
 *   handed anything.
 * What a placed record adds (64-bit signed arithmetic).  a = pos[L.entry_first];  d = L.pos_last >= L.pos_first ?
 *   L.pos_last - L.pos_first : 0;  k the database's k-mer length.  Forward (strand 0): lo = a, hi = a + d + k - 1.  Reverse
 *   (strand 1): lo = max(0, a - d), hi = a + k - 1.  With g = L.org: b_lo = min(lo / W, span_bins[g] - 1) and b_hi =
 *   min(hi / W, span_bins[g] - 1).  The record adds 1 to starts[g][b_lo] and 1 to depth[g][b] for every b in b_lo..b_hi.
 *   With diag_bin = 1 the interval [lo, hi] is exactly the genome interval covered by the chain's k-mers.
 * The pileup is a pure function of the multiset of placed records: it does not depend on the order of the records, the
 *   split into calls or the stream, is byte-identical across runs, and the pileup of a union is the element-wise sum of
 *   the pileups of the parts.
 * Summary.  One kid_pileup_rec per organism:
 *   n_placed        the sum of starts over the organism's bins         span_bins  as above
 *   bins_covered    bins with depth >= 1
 *   max_gap         the longest run of consecutive bins 0..span_bins-1 with depth = 0 (span_bins when nothing is placed)
 *   max_depth, max_depth_bin    the largest depth and the lowest bin that reaches it (0 when nothing is placed)
 *   max_starts, max_starts_bin  the same for starts
 *   reserved        0                                                   depth_sum  the sum of depth over the bins
 *   An organism without entries has an all-zero record.  The record is 48 bytes: nine uint32, four bytes of padding (zero)
 *   that align the uint64, and depth_sum.
 * Worked case.  W = 100, k = 30, organism 3 with entries at positions 0, 100, 250, 990: span_bins = 10.  Under
 *   (min_chain, min_margin) = (2, 1):  forward, entry_first at pos 100, pos_first 10, pos_last 130, n_chain 5, n_other 0:
 *   [lo, hi] = [100, 249], bins 1..2;  reverse, entry_first at pos 250, pos_first 0, pos_last 120, n_chain 3, n_other 2:
 *   [130, 279], bins 1..2;  forward, entry_first at pos 990, pos_last - pos_first = 100, n_chain 2, n_other 2: the margin is 0,
 *   not placed.  The third once more under (2, 0): [990, 1119], both ends clamp to bin 9.  Then
 *   starts = [0,2,0,0,0,0,0,0,0,1], depth = [0,2,2,0,0,0,0,0,0,1], record 3, 10, 3, 6, 2, 1, 2, 1, 0, depth_sum 5.
 * Storage.  depth is kept as a step array of B + n_orgs uint32: organism g owns the span_bins[g] + 1 slots from
 *   bin_base[g] + g on, a record adds +1 at slot b_lo and -1 (wrap-around) at slot b_hi + 1, and depth is the running sum.
 *   kid_pileup_export and kid_pileup_merge move (starts, steps): both are linear, merge adds element-wise.
 * Lifetime.  The database must outlive the pileup.  A pileup's geometry is that of the sites in force when it was made:
 *   after a later kid_db_set_sites (the clearing form included) kid_pileup_add* return KID_ERR_STATE, while summary, bins,
 *   export, counts and reset keep working on what it holds (it keeps the old site arrays alive; nothing freed is read).
 *   After kid_db_destroy of its database a pileup may only be passed to kid_pileup_destroy.
 * Calls.  A null pointer is KID_ERR_ARG.  kid_pileup_create: bin_width = 0 KID_ERR_ARG, then a database without sites
 *   KID_ERR_STATE (nothing allocated or launched), then B over the cap KID_ERR_ARG.  kid_pileup_add*: min_chain = 0
 *   KID_ERR_ARG, a stale pileup KID_ERR_STATE, n = 0 KID_OK with nothing launched.  kid_pileup_add_device (d_loci:
 *   kid_locus[n] in HBM) is asynchronous on `stream`; every reading call (counts, summary, bins, export, time) first waits
 *   for the pileup's own queued adds.  kid_pileup_bins with starts = depth = NULL and cap = 0 is the sizing call (bin_base
 *   alone is written; B is bin_base[n_orgs]); one array without the other, or cap < B, is KID_ERR_ARG and nothing is
 *   written.  kid_pileup_time: device time of the add kernels alone since the last query.  Calls on one pileup from
 *   several threads are serialised.                                                                                   */
typedef struct kid_pileup kid_pileup;
typedef struct kid_pileup_rec {
    uint32_t n_placed, span_bins, bins_covered, max_gap, max_depth, max_depth_bin, max_starts, max_starts_bin, reserved;
    uint64_t depth_sum; /* at offset 40 */
} kid_pileup_rec;
int kid_pileup_create(kid_db *db, uint32_t bin_width, kid_pileup **out);
int kid_pileup_destroy(kid_pileup *p);
int kid_pileup_info(kid_pileup *p, uint32_t *n_orgs, uint64_t *n_bins, uint32_t *bin_width);
int kid_pileup_reset(kid_pileup *p);
int kid_pileup_add(kid_pileup *p, const kid_locus *loci, uint64_t n, uint32_t min_chain, uint32_t min_margin);
int kid_pileup_add_device(kid_pileup *p, const void *d_loci, uint64_t n, uint32_t min_chain, uint32_t min_margin, void *stream);
int kid_pileup_counts(kid_pileup *p, uint64_t *n_records, uint64_t *n_placed);
int kid_pileup_summary(kid_pileup *p, kid_pileup_rec *out /* [n_orgs] */);
int kid_pileup_bins(kid_pileup *p, uint64_t *bin_base /* [n_orgs + 1] */, uint32_t *starts, uint32_t *depth, uint64_t cap);
int kid_pileup_export(kid_pileup *p, uint32_t *starts /* [B] */, uint32_t *steps /* [B + n_orgs] */);
int kid_pileup_merge(kid_pileup *p, const uint32_t *starts, const uint32_t *steps, uint64_t n_records, uint64_t n_placed);
int kid_pileup_time(kid_pileup *p, double *device_ms, uint64_t *calls, uint64_t *records);
/* Fragments into the same pileup: kid_fragment_locus records carry their org and interval themselves.  A record L is
 * placed when L.mates is in 1..3, paired_only = 0 or L.mates = 3, L.n_chain >= min_chain, (L.n_chain >= L.n_other ?
 * L.n_chain - L.n_other : 0) >= min_margin, L.org < n_orgs and span_bins[L.org] >= 1, and L.lo <= L.hi; otherwise it changes
 * nothing.  A placed record adds 1 to starts[g][b_lo] and 1 to depth[g][b] for b_lo..b_hi with g = L.org, b_lo = min(L.lo /
 * W, span_bins[g] - 1) and b_hi = min(L.hi / W, span_bins[g] - 1): the same step array and three atomics as a read.
 * n_records and n_placed count as for kid_pileup_add; the statuses are those of kid_pileup_add*; fragment records and read
 * records may be added to one pileup, whose counters are then the sums.
 * Worked case, on the pileup's own above (W = 100, organism 3 with span_bins = 10), under (min_chain, min_margin) = (2, 1):
 *   mates 3, n_chain 3, n_other 1, [lo, hi] = [100, 429]: bins 1..4;  mates 1, n_chain 2, n_other 0, [100, 159]: bin 1;
 *   mates 3, n_chain 2, n_other 2: the margin is 0, not placed;  mates 0: not placed.  Then starts = [0,2,0,0,0,0,0,0,0,0],
 *   depth = [0,2,1,1,1,0,0,0,0,0], n_records 4, n_placed 2.  With paired_only = 1 the second is not placed either.     */
int kid_pileup_add_fragments(kid_pileup *p, const kid_fragment_locus *recs, uint64_t n, uint32_t min_chain, uint32_t min_margin,
                             int paired_only);
int kid_pileup_add_fragments_device(kid_pileup *p, const void *d_recs, uint64_t n, uint32_t min_chain, uint32_t min_margin, int paired_only,
                                    void *stream);

/* ---- results -----------------------------------------------------------------
 * gcount[ntar], ucount[ntar] as written to <prefix>_result.txt (:1040-1043).
 * Synchronises the sample's outstanding work first.  The sample has ended then:
 * a kid_classify_* call or a tally into it is KID_ERR_STATE (and counts nothing)
 * until kid_sample_reset; the counters may be read again in any way.             */
int kid_sample_end(kid_sample *s, int64_t *gcount, int64_t *ucount);
/* The same for ONE sample whose batches were dealt out over n DISTINCT kid_sample objects (a sample named twice is
 * KID_ERR_ARG: its reads would count twice), one per GPU, each on its own replica of the database (kid_db_replicate):
 * gcount summed, ucount from the union of the seen-bitmaps (copied peer to peer to samples[0]'s GPU).  Replaces the
 * per-sample reset + write of main (newkmer_10nx.cpp:1015-1045) around N devices; the result is identical for any N
 * and any way of dealing the batches.                                                                           */
int kid_sample_end_merged(kid_sample **samples, int n, int64_t *gcount, int64_t *ucount);
/* {reads, k-mer lookups, table cells read, k-mer hits} so far (synchronises) */
int kid_sample_stats(kid_sample *s, uint64_t out[4]);

/* Kernel timing for benchmarks: when enabled, every batch records a HIP event pair around its
 * kid_classify_kernel launches (on the launch stream).  kid_sample_kernel_time synchronises, adds
 * up the elapsed times since the last call and returns the number of batches they belong to.  */
int kid_sample_set_timing(kid_sample *s, int enabled);
int kid_sample_kernel_time(kid_sample *s, double *total_ms, uint64_t *launches);
/* The same event pairs one by one: the milliseconds of every timed batch since the last call of THIS function, oldest
 * first (the two queries do not take from each other; a sample that is never asked keeps the latest 65536).  *n = how
 * many there are; the first min(cap, *n) are written to ms, and all of them count as reported.  Synchronises. */
int kid_sample_kernel_times(kid_sample *s, double *ms, uint64_t cap, uint64_t *n);
/* The same interval on the device's own clock, always on: the first workgroup of kid_classify_kernel to
 * start and the last one to finish stamp the 100 MHz realtime counter.  Sum over the batches since
 * the last call (or kid_sample_reset) and their number.  No event overhead, comparable with a
 * rocprofv3 kernel trace.                                                                      */
int kid_sample_kernel_time_device(kid_sample *s, double *total_ms, uint64_t *launches);

/* ---- multi-GPU merge helpers (reads sharded over ranks, DB replicated) ---------
 * ucount is |distinct DB k-mers hit| and is not additive over shards: ranks
 * exchange slices of the "seen" bitmap, OR them, and count their slice.  The bitmap
 * has one bit per DB ENTRY: bit o = "the key whose first insert was entry o (the o-th
 * (key, target) pair handed to kid_db_build) was hit".  It does not depend on where the
 * builder placed the cells, so bitmaps of samples on different kid_db objects built
 * from the same entries (one per GPU, either placement) can be OR-ed.              */
int kid_sample_seen_bytes(const kid_sample *s, uint64_t *nbytes);
int kid_sample_seen_export(kid_sample *s, uint64_t byte_off, uint64_t nbytes, void *dst, int dst_on_device);
int kid_sample_seen_or(kid_sample *s, uint64_t byte_off, uint64_t nbytes, const void *src, int src_on_device);
int kid_sample_gcount(kid_sample *s, int64_t *gcount);
/* ucount contribution of the bitmap bits (entry ordinals) [bit_begin, bit_end): multiples of 128, at most
 * 8 * kid_sample_seen_bytes (byte ranges of the bitmap helpers above are multiples of 16) */
int kid_sample_ucount_range(kid_sample *s, uint64_t bit_begin, uint64_t bit_end, int64_t *ucount);

/* ---- k-mer depth per database entry -------------------------------------------------
 * gcount says how many reads a target got and ucount how many of its database k-mers were hit at all.  With
 * KID_OPT_ENTRY_DEPTH on, a sample also counts HOW OFTEN each was hit: depth[o], one uint32 per database entry in the
 * numbering of the seen-bitmap and of kid_hit.entry.  A target whose hits are spread evenly over its k-mers is an organism
 * that is there, and its depth is its abundance; a handful of k-mers hit thousands of times is a conserved or
 * contaminating region.
 * Depth is counted by tallies alone: when kid_db_read_support / kid_db_read_support_fastq gets such a sample as `tally`,
 * every hit with target > 1 of every read it counts with confident > 0 adds 1 to depth[entry] -- exactly the hits whose
 * seen bit the tally sets; a k-mer that occurs twice in a read adds 2.  kid_classify_* into the same sample add no depth
 * (they do not visit hits one by one), so for a sample that was only tallied depth[o] > 0 exactly where seen bit o is set.
 * Counters saturate at 2^32 - 1.  gcount, ucount and the bitmap of the sample are what they are with the option off.
 * With the option off the calls below return KID_ERR_STATE and nothing is allocated, launched or compared anywhere.
 * All of them synchronise the sample's queued work first; none changes gcount, the bitmap or whether the sample has
 * ended, and they may be called before or after kid_sample_end.
 *   kid_sample_depth_export    the counters of the entries [entry_begin, entry_begin + n) -> dst (uint32[n], host or device);
 *                              a range beyond the database's n_entries is KID_ERR_ARG
 *   kid_sample_depth_add       a saturating add of src (uint32[n]) onto the same range: the companion of kid_sample_seen_or
 *                              and, with the export, the building block of a one-process-per-GPU merge
 *   kid_sample_depth_spectrum  bins in 2..4096 (KID_ERR_ARG beyond); every output is nullable
 *       spectrum[ntar * bins]  spectrum[t * bins + b] = the entries o with targets[o] == t and depth[o] == b for
 *                              b < bins - 1; the last column counts depth[o] >= bins - 1.  Column 0 holds the entries never
 *                              hit (duplicates of an earlier key and target-0 entries among them): a row sums to the
 *                              number of entries of that target handed to the builder
 *       ksum[ntar]             the sum of depth over the target's entries
 *       dmax[ntar]             the largest depth among them
 *                              It does not change the sample and may be repeated.
 *   kid_sample_depth_spectrum_merged  the same for ONE input sample dealt over n DISTINCT kid_sample objects on replicas
 *                              (a sample named twice: KID_ERR_ARG), every one with the option on: the counters are summed
 *                              with saturation into scratch on samples[0]'s device and the spectrum is that of the sum.  No
 *                              sample's counters change; a second call returns the same.                                */
int kid_sample_depth_export(kid_sample *s, uint64_t entry_begin, uint64_t n, void *dst, int dst_on_device);
int kid_sample_depth_add(kid_sample *s, uint64_t entry_begin, uint64_t n, const void *src, int src_on_device);
int kid_sample_depth_spectrum(kid_sample *s, uint32_t bins, uint64_t *spectrum, uint64_t *ksum, uint32_t *dmax);
int kid_sample_depth_spectrum_merged(kid_sample **samples, int n, uint32_t bins, uint64_t *spectrum, uint64_t *ksum, uint32_t *dmax);

/* ---- k-mers shared between samples ---------------------------------------------------
 * ucount says how many of a target's database k-mers a sample saw; two samples that both report 40 000 of 90 000 may
 * have seen the same 40 000 (one strain in both) or nearly disjoint sets (two strains).  What decides it is the
 * intersection of their seen-bitmaps, per target.  A bitmap is kid_sample_seen_bytes bytes in the layout of
 * kid_sample_seen_export: bit o (entry o as handed to the builder, with target T[o]) is bit o % 32 of the little-endian
 * 32-bit word o / 32.  For n bitmaps b_0 .. b_{n-1}
 *   shared[(i * n + j) * ntar + t] = #{ o in [0, n_entries) : bit o of b_i is set, bit o of b_j is set, T[o] == t }
 * -- a pure function of the bits and of T.  A bit at or beyond n_entries (the padding up to 128) is ignored, whatever it
 * holds; a bit a sample would never set (target 0 or 1, the duplicate of an earlier key) counts under its T[o] like any
 * other.  The matrix is symmetric and full; shared[i][i][t] is the number of bits of b_i under t, which for the bitmap
 * of a real sample is its ucount[t]; the same bitmap may be named twice.  Sums are 64-bit integers: the result does not
 * depend on any order of additions.  Jaccard and containment follow from shared and its diagonal.
 * One pass over the entries serves all pairs (kid_shared.hip.h): n * bytes + 4 * n_entries bytes are read once.
 *   bitmaps[n]   n in 1..KID_SHARED_MAX_SAMPLES (KID_ERR_ARG beyond, and for a null pointer); all in host memory
 *                (on_device = 0) or all in the memory of the database's device (1: 16-byte aligned, and at rest)
 *   shared       host memory, int64[n * n * ntar]; nothing is written to it when the call fails on its arguments
 * kid_db_shared_kmers is one of the calls of a kid_db that run one after the other (kid_db_read_hits above).  Both calls
 * synchronise before they return; neither touches a sample; their scratch (a device copy of host bitmaps, the matrix)
 * lives for the call.
 * kid_shared_kmers is the same without a kid_db, for a tool that has the probes but needs no table: targets[n_entries] in
 * host memory, as handed to kid_db_build (a targets[o] >= ntar: KID_ERR_TARGET); the bitmaps have the padded size a
 * kid_db of n_entries would report, ((n_entries + 127) / 128) * 16 bytes, 16 for no entries.
 * kid_shared_kmers_time: device time (HIP events) of the kernels of both calls, in this process, since the last query,
 * and the number of calls; copies and the clearing of the matrix are not in it.                                        */
#define KID_SHARED_MAX_SAMPLES 64
int kid_db_shared_kmers(kid_db *db, const void *const *bitmaps, int n, int on_device, int64_t *shared);
int kid_shared_kmers(int device, const uint32_t *targets, uint64_t n_entries, int32_t ntar, const void *const *bitmaps,
                     int n, int on_device, int64_t *shared);
int kid_shared_kmers_time(double *device_ms, uint64_t *calls);

/* ---- breadth of coverage per organism -------------------------------------------------
 * ucount says how many of a target's database k-mers a sample saw, not WHERE on the genome they lie.  An organism that
 * is present leaves its k-mers spread over its whole genome; a conserved gene, a transferred island or a contaminated
 * assembly leaves them on one locus.  Every probe line is SEQ,target,org,position,strand,count: entry o carries the
 * organism org[o] and the position pos[o] of the line it came from (a line of more than k bases yields several entries,
 * each with the line's two values unchanged).  With a bin width of W >= 1 bases:
 *   bin(o)          = pos[o] / W, as integers
 *   span_bins[g]    = 1 + max bin(o) over the entries of organism g, 0 when it has none
 *   B               = the sum of span_bins over the organisms: at most KID_COVERAGE_MAX_BINS, else KID_ERR_ARG before any
 *                     array of B elements is allocated
 *   probes[g][b]    = the entries of g in bin b;   seen_i[g][b] = those of them whose bit is set in bitmap i
 *   a bin is occupied when probes > 0
 * and per (bitmap i, organism g) one record, out[i * n_orgs + g]:
 *   n_probes        entries of g                     n_seen      entries of g with their bit set
 *   span_bins       as above (span_bins * W is roughly the genome length)
 *   bins            occupied bins                    bins_seen   bins with seen >= 1
 *   max_gap         take the occupied bins of g in ascending order: the longest run of consecutive elements of that
 *                   list with seen = 0.  Unoccupied bins neither break nor extend a run; bins when n_seen = 0
 *   max_bin_seen    the largest seen of any one bin  max_bin     the lowest bin that reaches it; 0 when n_seen = 0
 * Worked case: W = 1000, one organism with entries at 0, 10, 1500, 3999, 7000, 7001, 12000: bins 0,0,1,3,7,7,12,
 * span_bins 13, occupied [0,1,3,7,12], bins 5; with the bits of the entries at 10, 7000 and 7001 set, seen per occupied
 * bin is [1,0,0,2,0]: n_seen 3, bins_seen 2, max_gap 2 (bins 1 and 3: bin 2 is unoccupied and transparent),
 * max_bin_seen 2, max_bin 7.  An organism without entries has an all-zero record.
 * The result is a pure function of the bits, org, pos and W: it does not depend on the order of the entries, all values
 * are integers, and two runs give the same bytes.  Bits at or beyond n_entries are ignored, whatever they hold; a bit no
 * sample would set (a duplicate key, target 0 or 1) counts like any other (the convention of kid_shared_kmers); the same
 * bitmap may be named twice.
 *   org, pos     uint32[n_entries], host memory; an org[o] >= n_orgs is KID_ERR_ARG
 *   bitmaps[n]   n in 1..KID_SHARED_MAX_SAMPLES, host memory, each of the padded size a kid_db of n_entries would report:
 *                ((n_entries + 127) / 128) * 16 bytes, 16 for no entries
 *   out          host memory, kid_coverage[n * n_orgs]
 * A null pointer, n outside its range, bin_width = 0, an org out of range or B over the cap is KID_ERR_ARG, and nothing
 * is written.  n_entries = 0 is valid and gives all-zero records.  The calls are stateless like kid_shared_kmers (no
 * table is built, no sample is touched), take the bitmaps one after the other, synchronise before they return, and
 * their scratch lives for the call: 8 bytes per entry, one bitmap, 48 bytes per organism and 8 * B bytes.
 * kid_seen_coverage_bins is the per-bin profile, for plotting: bin_base[n_orgs + 1] (the bins of organism g are
 * bin_base[g] .. bin_base[g + 1] - 1), probes_per_bin[B] and seen_per_bin[n * B].  With probes_per_bin = seen_per_bin =
 * NULL and cap = 0 it is the sizing call: it writes *n_bins = B and bin_base.  Otherwise both arrays are given, cap is
 * the number of bins they have room for, and cap < B is KID_ERR_ARG.
 * kid_seen_coverage_time: device time (HIP events) of the kernels of both calls, in this process, since the last query,
 * and the number of calls; copies are not in it.                                                                      */
typedef struct kid_coverage {
    uint32_t n_probes, n_seen, span_bins, bins, bins_seen, max_gap, max_bin_seen, max_bin;
} kid_coverage;
#define KID_COVERAGE_MAX_BINS (1ull << 28)
int kid_seen_coverage(int device, const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs,
                      uint32_t bin_width, const void *const *bitmaps, int n, kid_coverage *out);
int kid_seen_coverage_bins(int device, const uint32_t *org, const uint32_t *pos, uint64_t n_entries, uint32_t n_orgs,
                           uint32_t bin_width, const void *const *bitmaps, int n, uint64_t *bin_base,
                           uint32_t *probes_per_bin, uint32_t *seen_per_bin, uint64_t cap, uint64_t *n_bins);
int kid_seen_coverage_time(double *device_ms, uint64_t *calls);

/* ---- probe-database builder ------------------------------------------------------------------------------------
 * Replaces the table of kmer_build_vf6.cpp (Hashtable, :132-215) and its three passes (process_seq, process_seq3,
 * process_seq2: :353-457, :553-640): 2^log2_cells uint32 cells, direct mapped by fmix64 of the canonical 30-mer, no key
 * stored; cell = target << 11 | count (0 = empty, 1 = spoiled).  Text is ACGTN, one byte per base (anything but A, C, G,
 * T breaks a k-mer); a call takes a whole sequence and streams it through the device in chunks of batch_bases.
 *   parent[ntar]   Tree1::parent after the add_edge calls (:81-97); entries in [0, ntar), else KID_ERR_TREE
 *   ntar           at most 2^21 (KID_ERR_ARG beyond: target << 11 overflows a cell)
 *   log2_cells     10..40; 35 is the reference's MAXHASH (128 GiB)
 *   batch_bases    k-mer positions per chunk (0 = 2^24)                                                            */
typedef struct kid_builder kid_builder;
typedef struct kid_build_cand {
    uint64_t key;      /* canonical 30-mer */
    int64_t gpos;      /* gpos_base + index of its last base in the text */
    int32_t target;    /* cell target (> 1) */
    uint16_t count;    /* cell count (>= minct[target]) */
    uint8_t strand_r;  /* 1: keyF >= keyR ('R'), 0: 'F' */
    uint8_t flags;     /* bit 0: check_entropy passes; bit 1: the k-mer is "bad" (printed, :546-548) */
} kid_build_cand;
/* free / total bytes of `device`'s memory (a 2^35-cell table needs 128 GiB) */
int kid_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);
int kid_builder_create(int device, int log2_cells, const int32_t *parent, int32_t ntar, uint64_t batch_bases, kid_builder **out);
void kid_builder_destroy(kid_builder *b);
/* phase 1, HashAdd (:168-193) for every 30-mer of text; target in [2, ntar) */
int kid_builder_add(kid_builder *b, const uint8_t *text, uint64_t len, int32_t target);
/* phase 2, HashRemove (:195-204) for every 30-mer of text */
int kid_builder_remove(kid_builder *b, const uint8_t *text, uint64_t len);
/* minct per target (:611-618), needed by kid_builder_claim; n = ntar */
int kid_builder_set_minct(kid_builder *b, const int32_t *minct, int32_t n);
/* phase 3, getHash (:206-213) over the text in order: every 30-mer reads its cell and sets it to 1.  out receives, in gpos
 * order, the occurrences that were the first to read a cell with target > 1 and count >= minct[target]; the caller applies
 * "gpos > minpos" and the MAXPROBES cap.  text[0] is at gpos_base; cap >= len - 29.  Sequences (orgs) must be claimed in
 * the reference's order.                                                                                           */
int kid_builder_claim(kid_builder *b, const uint8_t *text, uint64_t len, int64_t gpos_base, kid_build_cand *out, uint64_t cap,
                      uint64_t *n_out);
/* number of cells phase 1 filled (the reference's ht->size) */
int kid_builder_size(kid_builder *b, uint64_t *n_filled);
/* cells [first_cell, first_cell + n) of the table, for tests */
int kid_builder_export(kid_builder *b, uint64_t first_cell, uint64_t n, uint32_t *out);
/* the device's check_entropy flags (kid_build_cand.flags) for n keys, for tests */
int kid_builder_entropy(kid_builder *b, const uint64_t *keys, uint64_t n, uint8_t *flags);
/* device time (HIP events around the kernels) and bases handed over, per phase (add, remove, claim) */
int kid_builder_stats(kid_builder *b, double device_ms[3], uint64_t bases[3]);

/* (The synthetic workload generators, the random-gather probe and the device memory helpers that bench.py and the
 *  tests use live in kmer_id_amd_bench.h: they are not part of the boundary.)                                        */
#ifdef __cplusplus
}
#endif
#include "kmer_id_amd_bench.h"
#endif /* KMER_ID_AMD_H */
