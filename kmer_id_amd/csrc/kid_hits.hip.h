// kid_hits.hip.h -- every read's k-mer hits, in read-position order (kid_db_read_hits*).
// A hit = one k-mer window for which Hashtable::getHash returns a target > 0: the values process_read folds
// (newkmer_10nx.cpp:526-595).  The classify kernels fold them on the fly and keep the result alone; these kernels hand
// the list out: {position in the read, target, entry ordinal} per hit, CSR over the reads of the batch.
//
// The reads come as the descriptors of kid_prepare_kernel / kid_prepare_fastq_kernel, i.e. trimming, the "stop - start
// >= k" rule and the range checks are decided by the code that decides them for the classify path.  A read is cut into
// tiles of 64 consecutive windows; one wave takes a tile, one lane a window (text packed in registers, minimizers staged
// in LDS: the tile of kid_tile.hip.h at wave size, so that a 121-window read costs two tiles, not one of 256).
//
//   kid_hits_scan_*          tiles per read -> first tile of every read                       (exclusive scan)
//   kid_hits_count_kernel    every window is looked up ONCE; a tile leaves the 64-bit mask of its hit lanes
//   kid_hits_scan_*          popcount(mask) per tile -> first hit of every tile                (exclusive scan)
//   kid_hits_offsets_kernel  hit_offsets[r] = first hit of read r's first tile
//   kid_hits_fill_kernel     the lanes named by a mask look their key up again and store their hit at
//                            (first hit of the tile) + (hits in lower lanes): ordered, no atomics, no sort
//
// "Stage, scan, place" with 8 bytes staged per tile: the table is read once for the windows that miss (99 % of a
// metagenomic sample) and twice for those that hit.  Staging the hits themselves would cost 768 bytes of scratch per
// tile whatever it holds (3 GB for 2 M reads); counting and filling blindly would read every line twice.
// Everything is integer and every output place is a pure function of the batch: the result is byte-identical across
// runs, across any split of the reads into calls and across table geometries.
#pragma once
#include "kid_tile.hip.h"

#define KID_HITS_TILE 64u        // windows per tile = lanes per wave
#define KID_HITS_WAVE_TILES 4u   // consecutive tiles a wave takes per round (one search for the read of the first)
#define KID_HITS_WG_TILES (4u * KID_HITS_WAVE_TILES)
#define KID_HITS_SCAN_BLOCK 1024u // elements a workgroup of the scan kernels takes at a time

struct KidHit {
    uint32_t pos, target, entry;
};

// ------------------------------------------------------------------ exclusive scans over the batch
// out[i] = sum of src[0 .. i), out[n] = the total; 64-bit sums (a batch may hold 2^31 reads of 2^31 windows).
// Three small kernels: scan inside blocks of 1024, scan of the block totals by one workgroup, add.
// SRC 0: tiles of read i (from its descriptor); SRC 1: hits of tile i (popcount of its mask); SRC 2: the uint64 src[i]
// itself (kid_segments.hip.h: segments of read i, scanned in place).
// n is on the host (reads) or on the device (tiles: only the device knows how many a batch resident in HBM has).
template <int SRC>
__device__ __forceinline__ uint64_t kid_hits_scan_src(const void *src, uint64_t i)
{
    if (SRC == 0) {
        const int32_t nk = static_cast<const KidReadDesc *>(src)[i].n_kmers;
        return nk > 0 ? ((uint64_t)(uint32_t)nk + KID_HITS_TILE - 1u) / KID_HITS_TILE : 0ull;
    }
    if (SRC == 2) return static_cast<const uint64_t *>(src)[i];
    return (uint64_t)__popcll(static_cast<const unsigned long long *>(src)[i]);
}

template <int SRC>
__global__ __launch_bounds__(256) void kid_hits_scan_local_kernel(const void *src, const uint64_t *n_dev, uint64_t n_host, uint64_t *out,
                                                                   uint64_t *bsum, uint32_t *zero /* nullable: [n] cleared on the way */)
{
    __shared__ uint64_t wave_tot[4];
    const uint64_t n = n_dev ? *n_dev : n_host;
    const uint64_t nblk = (n + KID_HITS_SCAN_BLOCK - 1u) / KID_HITS_SCAN_BLOCK;
    for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint64_t i0 = blk * KID_HITS_SCAN_BLOCK + 4u * threadIdx.x;
        uint64_t x[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            x[j] = i0 + j < n ? kid_hits_scan_src<SRC>(src, i0 + j) : 0ull;
            if (zero && i0 + j < n) zero[i0 + j] = 0u;
        }
        const uint64_t upto = kid_block_exscan4(x, wave_tot);
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) out[i0 + j] = x[j];
        if (threadIdx.x == 255u) bsum[blk] = upto;
        __syncthreads(); // wave_tot[] is rewritten by the next round
    }
}

// (limit / over: a total above `limit` -- more tiles than the scratch was sized for: reads that overlap in the text, or a
//  text longer than the caller said -- is reported in *over and replaced by 0: the batch then has no tile and no hit)
__global__ __launch_bounds__(1024) void kid_hits_scan_top_kernel(uint64_t *bsum, const uint64_t *n_dev, uint64_t n_host, uint64_t *total,
                                                                  uint64_t limit, unsigned long long *over /* nullable */)
{
    __shared__ uint64_t wave_tot[16];
    const uint64_t n = n_dev ? *n_dev : n_host;
    const uint64_t nblk = (n + KID_HITS_SCAN_BLOCK - 1u) / KID_HITS_SCAN_BLOCK;
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < nblk; c0 += 1024u) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < nblk ? bsum[i] : 0ull;
        const uint64_t inc = kid_wave_incscan(v);
        if ((threadIdx.x & 63u) == 63u) wave_tot[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint64_t before = 0, tot = 0;
        for (uint32_t w = 0; w < 16u; w++) {
            const uint64_t c = wave_tot[w];
            if (w < (threadIdx.x >> 6)) before += c;
            tot += c;
        }
        if (i < nblk) bsum[i] = carry + before + inc - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (over && carry > limit) { *over += 1ull; carry = 0; }
        *total = carry;
    }
}

__global__ void kid_hits_scan_add_kernel(uint64_t *out, const uint64_t *bsum, const uint64_t *n_dev, uint64_t n_host, const uint64_t *total)
{
    const uint64_t n = n_dev ? *n_dev : n_host;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] += bsum[i / KID_HITS_SCAN_BLOCK];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *total;
}

// ------------------------------------------------------------------ the two passes over the tiles
// What both passes share: which read a tile belongs to and the tile's text.  A workgroup takes KID_HITS_WG_TILES
// consecutive tiles per round, a wave KID_HITS_WAVE_TILES of them: one binary search over tile_off[] for the first,
// a walk for the rest.  The barriers are workgroup-wide (every wave runs every round; tiles beyond the last are idle).
struct KidHitsTiles {
    const uint8_t *bases;       // 16-byte aligned; readable up to the end of the 16-byte chunk that holds the last base
    const KidReadDesc *desc;
    const uint64_t *tile_off;   // [n_reads + 1]: first tile of read r; [n_reads] = tiles of the batch
    uint64_t n_reads;
    unsigned long long *tile_mask; // [tiles]: lanes (windows) of the tile that hit
    unsigned long long *tile_valid; // nullable; [tiles]: lanes of the tile that hold a k-mer (kid_segments.hip.h asks for it)
};

// the read of tile t: tile_off[r] <= t < tile_off[r + 1] (reads without a window own no tile)
__device__ __forceinline__ uint64_t kid_hits_read_of(const KidHitsTiles &a, uint64_t t)
{
    uint64_t lo = 0, hi = a.n_reads; // tile_off[lo] <= t < tile_off[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a.tile_off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Pass 1: every window looked up once.  tile_mask[t] = its hit lanes; n_kmers[r] += the windows of the tile that hold
// a k-mer (no base that is not ACGTacgt(Uu): the read's share of the classify path's "lookups").
__global__ __launch_bounds__(256) void kid_hits_count_kernel(const KidDevDb db, const KidHitsTiles a, uint32_t *n_kmers /* nullable, zeroed */)
{
    __shared__ uint32_t W[4][8], IM[4][8], mm[4][KID_HITS_TILE + 16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t n_tiles = a.tile_off[a.n_reads];
    for (uint64_t base = (uint64_t)blockIdx.x * KID_HITS_WG_TILES; base < n_tiles; base += (uint64_t)gridDim.x * KID_HITS_WG_TILES) {
        uint64_t t = base + wv * KID_HITS_WAVE_TILES;
        uint64_t r = t < n_tiles ? kid_hits_read_of(a, t) : 0ull;
        for (uint32_t q = 0; q < KID_HITS_WAVE_TILES; q++, t++) {
            const bool active = t < n_tiles; // wave-uniform
            uint64_t p0 = 0, end = 0;
            if (active) {
                while (a.tile_off[r + 1] <= t) r++;
                const KidReadDesc d = a.desc[r];
                p0 = d.first_base + (t - a.tile_off[r]) * KID_HITS_TILE; // the tile's first window
                end = d.first_base + (uint64_t)(uint32_t)d.n_kmers;
                kid_tile_stage<KID_HITS_TILE, 8u>(a.bases, db, p0, end, lane, W[wv], IM[wv]);
            }
            __syncthreads();
            if (active && db.minloc) kid_tile_mmers<KID_HITS_TILE>(db, W[wv], p0, end, lane, mm[wv]);
            __syncthreads();
            if (active) {
                const uint64_t p = p0 + lane;
                bool valid = false, hit = false;
                if (p < end && kid_tile_is_kmer(IM[wv], p0 >> 4, p, db.k)) {
                    valid = true;
                    uint32_t slot = 0, nc = 0;
                    hit = kid_tile_lookup(db, W[wv], p0 >> 4, p, mm[wv] + lane, slot, nc) > 0;
                }
                const unsigned long long hm = __ballot(hit), vm = __ballot(valid);
                if (lane == 0) {
                    a.tile_mask[t] = hm;
                    if (a.tile_valid) a.tile_valid[t] = vm;
                    if (n_kmers && vm) atomicAdd(&n_kmers[r], (uint32_t)__popcll(vm));
                }
            }
            __syncthreads(); // W, IM and mm are free for the next tile
        }
    }
}

// hit_offsets[r] = first hit of read r's first tile ([n_reads] = the batch's hits, also to *n_hits)
__global__ void kid_hits_offsets_kernel(const uint64_t *tile_off, const uint64_t *tile_hit_off, uint64_t n_reads, uint64_t *hit_offsets,
                                        uint64_t *n_hits /* nullable */)
{
    const uint64_t n_tiles = tile_off[n_reads]; // (0 for a batch whose tiles did not fit: every offset is 0 then)
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r <= n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t t = tile_off[r];
        const uint64_t h = tile_hit_off[t < n_tiles ? t : n_tiles];
        hit_offsets[r] = h;
        if (r == n_reads && n_hits) *n_hits = h;
    }
}

// Pass 2: the lanes a tile's mask names look their key up again (the same function of the same table: the same answer,
// now with the cell's entry ordinal kept) and store their hit.  Tiles without a hit cost their mask.  Nothing is
// written when the batch has more hits than `cap`.
__global__ __launch_bounds__(256) void kid_hits_fill_kernel(const KidDevDb db, const KidHitsTiles a, const uint64_t *tile_hit_off,
                                                             const uint64_t *offsets /* read origins, or */, const KidFastqRec *recs,
                                                             KidHit *hits, uint64_t cap)
{
    __shared__ uint32_t W[4][8];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t n_tiles = a.tile_off[a.n_reads];
    if (tile_hit_off[n_tiles] > cap) return;
    for (uint64_t base = (uint64_t)blockIdx.x * KID_HITS_WG_TILES; base < n_tiles; base += (uint64_t)gridDim.x * KID_HITS_WG_TILES) {
        uint64_t t = base + wv * KID_HITS_WAVE_TILES;
        uint64_t r = 0;
        bool searched = false;
        for (uint32_t q = 0; q < KID_HITS_WAVE_TILES; q++, t++) {
            const unsigned long long hm = t < n_tiles ? a.tile_mask[t] : 0ull; // wave-uniform
            uint64_t p0 = 0;
            if (hm) {
                if (!searched) { r = kid_hits_read_of(a, t); searched = true; }
                while (a.tile_off[r + 1] <= t) r++;
                const KidReadDesc d = a.desc[r];
                p0 = d.first_base + (t - a.tile_off[r]) * KID_HITS_TILE;
                kid_tile_stage<KID_HITS_TILE, 8u>(a.bases, db, p0, d.first_base + (uint64_t)(uint32_t)d.n_kmers, lane, W[wv], nullptr);
            }
            __syncthreads();
            if ((hm >> lane) & 1ull) {
                const uint64_t p = p0 + lane;
                uint32_t slot = 0, nc = 0;
                const uint32_t tgt = kid_dev_lookup(db, kid_tile_key(W[wv], p0 >> 4, p, db.k), slot, nc); // (no strip here)
                const uint64_t origin = offsets ? offsets[r] : (uint64_t)recs[r].seq_off;
                KidHit h;
                h.pos = (uint32_t)(p - origin);
                h.target = tgt;
                h.entry = slot;
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
                hits[tile_hit_off[t] + rank] = h;
            }
            __syncthreads();
        }
    }
}
