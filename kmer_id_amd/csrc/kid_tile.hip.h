// kid_tile.hip.h -- what the kernels beside the classify path share: a tile of one record's windows (kid_long.hip.h at
// 256 windows per workgroup, kid_hits.hip.h at 64 per wave) and the ordered fold of a wave's hits (kid_long.hip.h,
// kid_support.hip.h).  None of it is on the path the benchmark measures; kid_classify_kernel has forms of its own, held
// in registers.
//
// A tile = TILE consecutive windows of one record, the first at base p0 (absolute index in the batch text).  Its text
// is staged as packed words of 16 bases, word 0 = the chunk c0 = p0 >> 4 that holds p0.  A position p of the tile is
// read through kid_tile_window, which takes the three words from (p >> 4) - c0 on.  The positions read are the windows
// p0 .. p0 + TILE - 1 and the m-mers p0 .. p0 + TILE + win - 2; with p0 & 15 <= 15 and win <= 17 (k <= 31) the last of
// them starts at most TILE + 30 bases into word 0, so words 0 .. (TILE + 30) / 16 + 2 are touched: KID_TILE_WORDS, 20
// for 256 windows and 8 for 64.  The m-mer strip holds TILE + win - 1 <= TILE + 16 hashes.  Text exists up to the chunk
// that holds the record's last base (of window `end - 1`: base end + k - 2): nothing beyond it is ever loaded, the words
// there are zero, and the window test and the m-mer clamp keep what they would spell from being used.
#pragma once
#include "kid_kernels.hip.h"

#define KID_TILE_WORDS(TILE) (((TILE) + 30u) / 16u + 3u)

// Stage the tile's words (and invalid-base masks; IM nullable) in the caller's LDS arrays of CHUNKS words each, by the
// threads j = 0 .. CHUNKS - 1 of the tile.  end = the record's first base + its windows.  The caller's barrier follows.
template <uint32_t TILE, uint32_t CHUNKS>
__device__ __forceinline__ void kid_tile_stage(const uint8_t *bases, const KidDevDb &db, uint64_t p0, uint64_t end, uint32_t j, uint32_t *W,
                                               uint32_t *IM)
{
    static_assert(CHUNKS >= KID_TILE_WORDS(TILE), "a window of the tile would read beyond the staged words");
    if (j < CHUNKS) {
        const uint64_t c0 = p0 >> 4, c_last = (end + (uint64_t)db.k - 2u) >> 4;
        uint32_t cw = 0, ci = 0;
        if (j < KID_TILE_WORDS(TILE) && c0 + j <= c_last) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bases + 16ull * (c0 + j));
            kid_pack16(v, db.u_is_t, cw, ci);
        }
        W[j] = cw;
        if (IM) IM[j] = ci;
    }
}

// 32 bases starting at `base`, first base in the top bits (c0 = chunk of the tile's first base)
__device__ __forceinline__ uint64_t kid_tile_window(const uint32_t *W, uint64_t c0, uint64_t base)
{
    const uint32_t w0 = (uint32_t)((base >> 4) - c0);
    const uint32_t o2 = (uint32_t)(base & 15u) * 2u;
    const uint64_t A = ((uint64_t)W[w0] << 32) | W[w0 + 1];
    const uint64_t B = W[w0 + 2];
    return (A << o2) | ((B << o2) >> 32);
}

// mm[q] = hashed m-mer of position p0 + q, q = 0 .. TILE + win - 2, clamped to the record's last m-mer; by the TILE
// threads j of the tile.  (Minimizer-localised tables alone: the reference placement has no minimizers.)
template <uint32_t TILE>
__device__ __forceinline__ void kid_tile_mmers(const KidDevDb &db, const uint32_t *W, uint64_t p0, uint64_t end, uint32_t j, uint32_t *mm)
{
    const uint32_t win = (uint32_t)kid_min_window(db.k);
    const int mlen = kid_min_mlen(db.k);
    const uint64_t last_m = end + (uint64_t)db.k - 1u - (uint64_t)mlen;
    for (uint32_t q = j; q < TILE + win - 1u; q += TILE) {
        uint64_t p = p0 + q;
        p = p < last_m ? p : last_m;
        mm[q] = kid_mmer_hash((uint32_t)(kid_tile_window(W, p0 >> 4, p) >> (64 - 2 * mlen)), mlen);
    }
}

// does window p hold a k-mer: one touching a base that is not ACGTacgt(Uu) holds none (newkmer_10nx.cpp:520-526,604)
__device__ __forceinline__ bool kid_tile_is_kmer(const uint32_t *IM, uint64_t c0, uint64_t p, int k)
{
    const uint32_t iw = (uint32_t)((p >> 4) - c0);
    uint64_t im = (uint64_t)IM[iw] | ((uint64_t)IM[iw + 1] << 16) | ((uint64_t)IM[iw + 2] << 32);
    im >>= (p & 15u);
    return (im & ((1ull << k) - 1ull)) == 0;
}

// the canonical key of window p
__device__ __forceinline__ uint64_t kid_tile_key(const uint32_t *W, uint64_t c0, uint64_t p, int k)
{
    return kid_canonical(kid_tile_window(W, c0, p) >> (64 - 2 * k), k);
}

// Key and lookup of window p -> its target (0: absent), entry ordinal and cells read.  mm_p = the window's place in
// the strip of kid_tile_mmers: its minimizer is the minimum of the `win` hashes from there on (not read for the
// reference placement, which has no strip).
__device__ __forceinline__ uint32_t kid_tile_lookup(const KidDevDb &db, const uint32_t *W, uint64_t c0, uint64_t p, const uint32_t *mm_p,
                                                    uint32_t &slot, uint32_t &ncell)
{
    const uint64_t key = kid_tile_key(W, c0, p, db.k);
    if (!db.minloc) return kid_dev_lookup(db, key, slot, ncell);
    const uint32_t win = (uint32_t)kid_min_window(db.k);
    uint32_t g = 0xFFFFFFFFu;
    for (uint32_t w = 0; w < win; w++) g = mm_p[w] < g ? mm_p[w] : g;
    return kid_bucket_lookup(db, key, g, slot, ncell);
}

// ------------------------------------------------------------------ the ordered fold of a wave's hits
// process_read's left fold (newkmer_10nx.cpp:588-595; msca is not associative) over the hits the lanes named by `rem`
// hold, in lane order, onto the running result uf (0: no hit yet; ufr = its ancestor row when ROWS).  tgt = the lane's
// hit (0: none), row = its row.  Every lane works out the step its own hit would make from the current result; the
// first lane that changes it is taken and everything up to it masked off: one round per change of the result, a
// handful per record, instead of one per hit.  Wave-uniform in uf, ufr and rem.
template <bool ROWS>
__device__ __forceinline__ void kid_jump_fold(const KidDevDb &db, uint32_t tgt, const uint4 &row, uint64_t rem, uint32_t &uf, uint4 &ufr)
{
    while (rem) {
        uint32_t rj = tgt;
        uint4 roj = row;
        if (uf != 0 && tgt != uf && tgt != 0) {
            if (ROWS) rj = kid_msca_rows(tgt, row, uf, ufr, roj);
            else rj = kid_msca_climb(db, tgt, uf);
        }
        const uint64_t ch = __ballot(rj != uf) & rem;
        if (!ch) break;
        const int jj = __builtin_ctzll(ch);
        uf = (uint32_t)__builtin_amdgcn_readlane((int)rj, jj);
        if (ROWS) ufr = kid_row_of_lane(roj, jj);
        rem &= jj >= 63 ? 0ull : ~((2ull << jj) - 1ull);
    }
}
