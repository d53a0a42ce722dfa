// kid_api_core.h -- what every area of the host library uses: the error record, KID_HIP, device selection, grids, and
// the host-side checks and uploads the classify and the read-hits entry points share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/kmer_id_amd.h"
#include "kid_own.h"

static thread_local std::string g_last_error;

static int kid_fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

#define KID_HIP(call)                                                                                              \
    do {                                                                                                           \
        hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess)                                                                                      \
            return kid_fail(e_ == hipErrorOutOfMemory ? KID_ERR_NOMEM : KID_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                            hipGetErrorString(e_), __FILE__, __LINE__);                                            \
    } while (0)

extern "C" const char *kid_strerror(int status)
{
    switch (status) {
    case KID_OK: return "ok";
    case KID_ERR_ARG: return "bad argument";
    case KID_ERR_NOMEM: return "out of memory";
    case KID_ERR_HIP: return "HIP runtime error";
    case KID_ERR_TABLE_FULL: return "out of memory in table";
    case KID_ERR_TREE: return "taxonomy parent[] is out of range or cyclic";
    case KID_ERR_NO_DEVICE: return "no HIP device";
    case KID_ERR_TARGET: return "target id outside [0, ntar)";
    case KID_ERR_IO: return "I/O error";
    case KID_ERR_FORMAT: return "malformed input";
    case KID_ERR_STATE: return "call sequence error";
    default: return "unknown status";
    }
}

extern "C" const char *kid_last_error(void) { return g_last_error.c_str(); }

extern "C" int kid_device_count(int *count)
{
    if (!count) return kid_fail(KID_ERR_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return kid_fail(KID_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return KID_OK;
}

static int kid_use_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return kid_fail(KID_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                        e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return kid_fail(KID_ERR_ARG, "device %d out of range [0,%d)", device, n);
    KID_HIP(hipSetDevice(device));
    return KID_OK;
}

static inline int kid_grid_for(uint64_t n, int block, int cap_blocks)
{
    uint64_t g = (n + (uint64_t)block - 1) / (uint64_t)block;
    if (g < 1) g = 1;
    if (g > (uint64_t)cap_blocks) g = (uint64_t)cap_blocks;
    return (int)g;
}

// ---------------------------------------------------------------- batches from host buffers
// The host's check of an offsets batch: monotone offsets, reads of at most 2^31-1 bytes, [start,stop] inside the read.
// *max_kmers: the largest n_kmers of the batch; *max_tiles (null: not wanted): a read of L bytes has at most L windows,
// i.e. at most L / tile + 1 tiles of `tile` windows, added up over the reads.
static int kid_check_offsets_batch(const uint64_t *offsets, const int32_t *start, const int32_t *stop, uint64_t n_reads, int k,
                                   int64_t *max_kmers, uint32_t tile, uint64_t *max_tiles)
{
    int64_t mk = 0;
    uint64_t mt = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (offsets[r + 1] < offsets[r]) return kid_fail(KID_ERR_ARG, "offsets not monotone at read %llu", (unsigned long long)r);
        const uint64_t len = offsets[r + 1] - offsets[r];
        const int64_t span = start ? (int64_t)stop[r] - (int64_t)start[r] + 1 : (int64_t)len;
        if (span - k + 1 > mk) mk = span - k + 1;
        if (len > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "read %llu longer than 2^31-1", (unsigned long long)r);
        if (start && start[r] <= stop[r] && (start[r] < 0 || (uint64_t)stop[r] >= len))
            return kid_fail(KID_ERR_ARG, "read %llu: [start,stop] = [%d,%d] outside the read of length %llu (string::at would throw)",
                            (unsigned long long)r, start[r], stop[r], (unsigned long long)len);
        if (max_tiles) mt += len / tile + 1;
    }
    *max_kmers = mk;
    if (max_tiles) *max_tiles = mt;
    return KID_OK;
}

// ... of a block of FASTQ text with the host's line index.  *max_tiles (null: not wanted) has the records' tiles added:
// they may share or overlap sequence bytes -- unless `masking` (a min_base_quality or low_complexity option is on: bases
// are overwritten in the device copy of the text, kid_mask.hip.h and kid_lowc.hip.h): then the lines must lie in
// ascending order without overlap, sequence, quality, next sequence, .., as every indexer of a real file leaves them, so that no byte one record
// writes is a byte any record's decision reads.  *longest (with `masking`): raised to the longest sequence line.
// mate: null, or "mate 1, " / "mate 2, " in front of the messages about one block of a call that has two (its caller has
// checked the size of both together; an absent mate, seq_len = qual_len = 0, has no line to be in order).
static int kid_check_fastq_block(const kid_fastq_rec *recs, uint64_t n_reads, uint64_t text_nbytes, uint32_t tile, uint64_t *max_tiles,
                                 bool masking = false, uint32_t *longest = nullptr, const char *mate = nullptr)
{
    if (!mate && text_nbytes >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "a FASTQ block of 4 GiB or more");
    const char *pre = mate ? mate : "";
    uint64_t free_from = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const kid_fastq_rec &c = recs[r];
        if ((uint64_t)c.seq_off + c.seq_len > text_nbytes || (uint64_t)c.qual_off + c.qual_len > text_nbytes)
            return kid_fail(KID_ERR_ARG, "%srecord %llu lies outside the text block", pre, (unsigned long long)r);
        if (max_tiles) *max_tiles += c.seq_len / tile + 1;
        if (masking && !(mate && c.seq_len == 0 && c.qual_len == 0)) {
            if (c.seq_off < free_from || (uint64_t)c.seq_off + c.seq_len > c.qual_off)
                return kid_fail(KID_ERR_ARG, "%srecord %llu: with min_base_quality or low_complexity on, the lines of a block must be in ascending order and "
                                             "must not overlap", pre, (unsigned long long)r);
            free_from = (uint64_t)c.qual_off + c.qual_len;
            if (longest && c.seq_len > *longest) *longest = c.seq_len;
        }
    }
    return KID_OK;
}

// The kernels read text in 16-byte groups and look a little past the last read: a device copy of `nbytes` of text has
// this many bytes, zero from the last whole group on.
static inline uint64_t kid_text_bytes(uint64_t nbytes) { return ((nbytes + 15) & ~15ull) + 32; }

// (src2: a second part that goes right behind the first, as one text)
static int kid_upload_text(const KidDevBuf &buf, const uint8_t *src, uint64_t nbytes, hipStream_t stream, const uint8_t *src2 = nullptr,
                           uint64_t nbytes2 = 0)
{
    const uint64_t all = nbytes + nbytes2, tail = all & ~15ull;
    KID_HIP(hipMemsetAsync(buf.as<uint8_t>() + tail, 0, kid_text_bytes(all) - tail, stream));
    if (nbytes) KID_HIP(hipMemcpyAsync(buf.p, src, nbytes, hipMemcpyHostToDevice, stream));
    if (nbytes2) KID_HIP(hipMemcpyAsync(buf.as<uint8_t>() + nbytes, src2, nbytes2, hipMemcpyHostToDevice, stream));
    return KID_OK;
}

// Offsets counted from the first read's first byte, which is where the uploaded text starts: the caller's own array
// when that is offset 0, else `rel`, filled here.  `rel` must stay alive until the copy that reads it is done.
static const uint64_t *kid_rebased_offsets(const uint64_t *offsets, uint64_t n_reads, std::vector<uint64_t> &rel)
{
    const uint64_t base0 = offsets[0];
    if (base0 == 0) return offsets;
    rel.resize(n_reads + 1);
    for (uint64_t r = 0; r <= n_reads; r++) rel[r] = offsets[r] - base0;
    return rel.data();
}

// ---------------------------------------------------------------- batches in device memory
static int kid_check_n_reads(uint64_t n_reads)
{
    if (n_reads > 0x7FFFFFFFull) return kid_fail(KID_ERR_ARG, "at most 2^31-1 reads per batch");
    return KID_OK;
}

// What every device form refuses about its batch, in the order callers see, and the KidBatch of the rest.  (The limit
// on n_reads is not here: the classify form meets it later, in kid_launch_classify, than the hit-pass forms do.)
static int kid_check_device_batch(const void *d_bases, const void *d_offsets, const void *d_start, const void *d_stop, uint64_t n_reads,
                                  KidBatch *b)
{
    if (n_reads && (!d_bases || !d_offsets)) return kid_fail(KID_ERR_ARG, "null argument");
    if (((uintptr_t)d_bases & 15u) != 0) return kid_fail(KID_ERR_ARG, "d_bases must be 16-byte aligned");
    if ((d_start == nullptr) != (d_stop == nullptr)) return kid_fail(KID_ERR_ARG, "start and stop must both be given or both be null");
    *b = KidBatch{};
    b->bases = (const uint8_t *)d_bases;
    b->offsets = (const uint64_t *)d_offsets;
    b->start = (const int32_t *)d_start;
    b->stop = (const int32_t *)d_stop;
    b->n = n_reads;
    return KID_OK;
}
