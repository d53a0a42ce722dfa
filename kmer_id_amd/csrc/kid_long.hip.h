// kid_long.hip.h -- very long records (FASTA contigs classified whole; KidLong* of kid_table.hip.h).
// A record is one left fold over its hits (newkmer_10nx.cpp:588-595; msca is not associative), which the classify
// kernels run inside ONE wave: 9.7 ms per megabase when the batch holds few records.  When the host sees few long
// records in a batch it hands them to two kernels instead:
//   kid_long_hits_kernel   every k-mer of every long record is looked up by a lane of its own, all over the chip; a hit
//                          leaves its target in hits[position] (and its bit in the seen-bitmap)
//   kid_long_fold_kernel   one workgroup per record compacts the hits in position order and folds them, 64 at a time,
//                          jumping from change to change of the running result (kid_jump_fold)
// Plain code: this path runs a few hundred times per batch, not a hundred million times.
#pragma once
#include "kid_tile.hip.h"

// The list -> the plan: where every long record's hits go.  One thread: the list is short.  A record that does not fit
// the hit array any more is handed back to the classify kernels (its descriptor gets its k-mers back).
__global__ void kid_long_plan_kernel(KidLongList *list, KidLongPlan *plan, KidReadDesc *desc, KidRareArgs *rare, uint32_t seq,
                                     uint64_t hits_cap, uint64_t tiles_cap)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t n = list->n < KID_LONG_MAX ? list->n : KID_LONG_MAX;
    uint64_t off = 0, tiles = 0;
    uint32_t m = 0, back = 0;
    for (uint32_t i = 0; i < n; i++) {
        const KidLongList::Item it = list->e[i];
        const uint64_t nt = ((uint64_t)it.n_kmers + 255u) / 256u;
        if (off + it.n_kmers > hits_cap || tiles + nt > tiles_cap) {
            desc[it.read].n_kmers = (int32_t)it.n_kmers;
            back = it.n_kmers > back ? it.n_kmers : back;
            continue;
        }
        KidLongRec r;
        r.first_base = it.first_base; r.hits_off = off; r.n_kmers = it.n_kmers; r.read = it.read; r.tile0 = tiles;
        plan->recs[m++] = r;
        off += it.n_kmers;
        tiles += nt;
    }
    plan->n_recs = m;
    plan->n_tiles = tiles;
    plan->total_kmers = off;
    list->n = 0; // for the batch that uses this set next
    if (back) { // (the kernels pick themselves by the longest read of the batch)
        const unsigned long long v = ((unsigned long long)seq << 32) | back;
        if (v > rare->batch_max) rare->batch_max = v;
    }
}

// Every k-mer of every long record is looked up by a lane of its own.  A tile = 256 consecutive k-mers of one
// record: its text is read as text (16 bytes per thread by the first 20 threads), packed in registers and staged in LDS
// (kid_tile.hip.h), like the classify kernels' general loops stage a segment.
__global__ __launch_bounds__(256) void kid_long_hits_kernel(const KidDevDb db, const uint8_t *bases, const KidLongPlan *plan,
                                                             uint32_t *hits, uint8_t *tile_any, uint32_t *seen,
                                                             unsigned long long *stats)
{
    __shared__ uint32_t mm[256 + 32];
    __shared__ uint32_t W[24], IM[24]; // the tile's packed words and invalid masks
    const uint32_t n_recs = plan->n_recs;
    const uint64_t n_tiles = plan->n_tiles;
    const KidLongRec *recs = plan->recs;
    unsigned long long n_lookups = 0, n_cells = 0, n_hits = 0;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // the record this tile belongs to (recs are few: binary search over tile0)
        uint32_t lo = 0, hi = n_recs;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (recs[mid].tile0 <= tile) lo = mid; else hi = mid; }
        const KidLongRec rc = recs[lo];
        const uint32_t j = threadIdx.x, i = (uint32_t)(tile - rc.tile0) * 256u + j; // this thread's k-mer within the record
        const uint64_t p = rc.first_base + i, p0 = p - j, end = rc.first_base + rc.n_kmers;
        kid_tile_stage<256u, 24u>(bases, db, p0, end, j, W, IM);
        __syncthreads();
        if (db.minloc) kid_tile_mmers<256u>(db, W, p0, end, j, mm); // (workgroup-uniform)
        __syncthreads();
        uint32_t hit_t = 0;
        if (i < rc.n_kmers && kid_tile_is_kmer(IM, p0 >> 4, p, db.k)) {
            uint32_t slot = 0, nc = 0;
            hit_t = kid_tile_lookup(db, W, p0 >> 4, p, mm + j, slot, nc);
            n_lookups++;
            n_cells += nc;
            if (hit_t > 0) n_hits++;
            if (hit_t > 1) atomicOr(&seen[slot >> 5], 1u << (slot & 31u));
        }
        if (i < rc.n_kmers) hits[rc.hits_off + i] = hit_t; // (every position: the array is not cleared between batches)
        const int any = __syncthreads_or(hit_t > 0 ? 1 : 0); // (also: mm[], W[] and IM[] are free for the next tile)
        if (threadIdx.x == 0) tile_any[tile] = any ? 1 : 0; // the fold skips tiles without hits unseen
    }
    // one set of atomics per workgroup (see kid_classify_kernel)
    __shared__ unsigned long long tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    if (n_lookups) atomicAdd(&tot[0], n_lookups);
    if (n_cells) atomicAdd(&tot[1], n_cells);
    if (n_hits) atomicAdd(&tot[2], n_hits);
    __syncthreads();
    if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd(&stats[1 + threadIdx.x], tot[threadIdx.x]);
}

__global__ __launch_bounds__(256) void kid_long_fold_kernel(const KidDevDb db, const KidLongPlan *plan, const uint32_t *hits,
                                                             const uint8_t *tile_any, unsigned long long *gcount,
                                                             uint32_t *out_final)
{
    if (blockIdx.x >= plan->n_recs) return; // (a grid of KID_LONG_MAX workgroups: the host does not know how many there are)
    const KidLongRec *recs = plan->recs;
    __shared__ uint32_t list[256];
    __shared__ uint32_t wcount[4];
    __shared__ uint8_t flags[256];
    const KidLongRec rc = recs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t uf = 0; // the running result (wave 0)
    uint4 ufr = make_uint4(0, 0, 0, 0);
    const uint32_t ntile = (rc.n_kmers + 255u) / 256u;
    for (uint32_t tg = 0; tg < ntile; tg += 256u) { // 256 tiles = 65 536 positions at a time: most hold no hit at all
      const uint32_t myt = tg + threadIdx.x;
      const uint8_t fl = myt < ntile ? tile_any[rc.tile0 + myt] : (uint8_t)0;
      flags[threadIdx.x] = fl;
      if (!__syncthreads_or(fl)) continue;
      for (uint32_t tt = 0; tt < 256u && tg + tt < ntile; tt++) {
        if (!flags[tt]) continue; // (workgroup-uniform)
        const uint32_t t0 = (tg + tt) * 256u;
        {
        const uint32_t i = t0 + threadIdx.x;
        const uint32_t h = i < rc.n_kmers ? hits[rc.hits_off + i] : 0u;
        const uint64_t bm = __ballot(h != 0);
        if (lane == 0) wcount[wv] = (uint32_t)__popcll(bm);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) { const uint32_t c = wcount[w]; if (w < wv) before += c; total += c; }
        if (h != 0) list[before + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u))] = h;
        __syncthreads();
        if (wv == 0) {
            for (uint32_t c0 = 0; c0 < total; c0 += 64u) {
                const uint32_t n = total - c0 < 64u ? total - c0 : 64u;
                const uint32_t tgt = lane < n ? list[c0 + lane] : 0u;
                const uint64_t rem = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
                if (db.rows) kid_jump_fold<true>(db, tgt, tgt ? db.rows[tgt] : make_uint4(0, 0, 0, 0), rem, uf, ufr);
                else kid_jump_fold<false>(db, tgt, make_uint4(0, 0, 0, 0), rem, uf, ufr);
            }
        }
        __syncthreads();
        }
      }
      __syncthreads(); // flags[] is rewritten by the next round
    }
    if (threadIdx.x == 0) {
        // the classify kernels counted the record under target 0 (they saw it without k-mers)
        if (uf != 0) {
            atomicAdd(&gcount[uf], 1ull);
            atomicAdd(&gcount[0], ~0ull); // - 1
        }
        if (out_final) out_final[rc.read] = uf;
    }
}
