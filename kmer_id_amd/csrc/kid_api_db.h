// kid_api_db.h -- the database handle: taxonomy preparation, the reference-order host table builder and the GPU one,
// replicas, and the unit entry points (lookup, msca, hash, trim).
#pragma once
#include <memory>
#include <mutex>
#include <stdlib.h>
#include <vector>

#include "kid_api_core.h"
#include "kid_build.hip.h"
#include "kid_kernels.hip.h"

// the sites of a database's entries (kid_db_set_sites, kid_api_loci.h): shared with the pileups made from them
// (kid_api_pileup.h), which keep the arrays they were made for alive behind a second kid_db_set_sites or kid_db_destroy
struct KidSites {
    KidDevBuf org, pos;  // uint32 per entry
    uint32_t n_orgs = 0; // the largest org + 1
};

struct kid_db {
    int device = 0;
    int num_cu = 0;
    KidDevDb d{}; // what the kernels get: the pointers below and the geometry
    KidDevBuf table, rows, parent, depth;
    KidDevBuf digest;       // uint2 per table line: the digest plane of a GPU-built minimizer-localised table (kid_common.h)
    KidDevBuf ord_target;  // uint32: target of entry o as handed to the builder, padded with zeros to a multiple of 128
    uint64_t seen_bits = 0; // entries rounded up to whole 16-byte groups of the seen-bitmap
    KidDevBuf entries_per_target; // unsigned long long [ntar]: made under hits_mu by the first depth spectrum (kid_api_depth.h)
    kid_db_info info{};
    std::unique_ptr<struct KidHitsState> hits; // scratch of kid_db_read_hits*, made by the first call (kid_api_hits.h)
    std::mutex hits_mu;
    int min_base_quality = 0; // KID_DB_OPT_MIN_BASE_QUALITY (kid_api_mask.h): read and written under hits_mu; a replica starts at 0
    int low_complexity = 0;   // KID_DB_OPT_LOW_COMPLEXITY (kid_api_lowc.h): the same rules
    std::shared_ptr<KidSites> sites; // kid_db_set_sites (kid_api_loci.h), under hits_mu; a replica starts without
    uint64_t sites_gen = 0;          // bumped by every kid_db_set_sites that takes effect, the clearing form included
    ~kid_db(); // kid_api_hits.h: where KidHitsState is complete
};
typedef std::unique_ptr<kid_db, void (*)(kid_db *)> KidDbPtr; // a database under construction

// a new database object on `device` (selected by the caller)
static KidDbPtr kid_db_new(int device)
{
    KidDbPtr db(new kid_db(), kid_db_destroy);
    db->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) db->num_cu = prop.multiProcessorCount;
    if (db->num_cu <= 0) db->num_cu = 256;
    return db;
}

// ---------------------------------------------------------------- taxonomy preparation
// effective parent = Tree1::get_parent (newkmer_10nx.cpp:146-152): nodes 0 and 1 answer root.
static int kid_prepare_tree(const int32_t *parent, int32_t ntar, std::vector<int32_t> &par, std::vector<int32_t> &depth,
                            int &max_depth)
{
    par.assign((size_t)ntar, 1);
    depth.assign((size_t)ntar, -1);
    for (int32_t i = 0; i < ntar; i++) {
        int32_t p = (i != 1 && i > 0) ? parent[i] : 1;
        if (p < 0 || p >= ntar) return kid_fail(KID_ERR_TREE, "parent[%d] = %d is outside [0,%d)", i, p, ntar);
        par[(size_t)i] = p;
    }
    depth[1] = 0;
    max_depth = 0;
    std::vector<int32_t> stack;
    for (int32_t i = 0; i < ntar; i++) {
        if (depth[(size_t)i] >= 0) continue;
        stack.clear();
        int32_t z = i;
        while (depth[(size_t)z] < 0) {
            if ((int32_t)stack.size() > ntar) return kid_fail(KID_ERR_TREE, "cycle in parent[] reachable from node %d", i);
            depth[(size_t)z] = -2; // on stack
            stack.push_back(z);
            z = par[(size_t)z];
            if (depth[(size_t)z] == -2) return kid_fail(KID_ERR_TREE, "cycle in parent[] reachable from node %d", i);
        }
        int32_t d = depth[(size_t)z];
        for (size_t j = stack.size(); j-- > 0;) depth[(size_t)stack[j]] = ++d;
    }
    for (int32_t i = 0; i < ntar; i++) max_depth = depth[(size_t)i] > max_depth ? depth[(size_t)i] : max_depth;
    return KID_OK;
}

static void kid_make_rows(const std::vector<int32_t> &par, const std::vector<int32_t> &depth, std::vector<uint4> &rows)
{
    const size_t ntar = par.size();
    rows.assign(ntar, make_uint4(0, 0, 0, 0));
    for (size_t i = 0; i < ntar; i++) {
        uint16_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int32_t d = depth[i];
        e[0] = (uint16_t)d;
        int32_t z = (int32_t)i;
        while (d >= 1) {
            if (d <= 7) e[d] = (uint16_t)z;
            z = par[(size_t)z];
            d--;
        }
        rows[i] = make_uint4((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                             (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16));
    }
}

// ---------------------------------------------------------------- host table builder
// Hashtable::add_kmer replayed in file order into 16-byte cells: the exact cell
// geometry of the reference, needed when lookups are probe-capped (kmer_read_m3).
static int kid_host_build(const uint64_t *keys, const uint32_t *targets, uint64_t n, int log2_slots, uint4 *cells,
                          uint64_t *n_occupied)
{
    const uint64_t nslots = 1ULL << log2_slots, mask = nslots - 1;
    uint64_t size = 0, occ = 0;
    for (uint64_t e = 0; e < n; e++) {
        const uint64_t key = keys[e], hash = kid_fmix64(key);
        uint64_t reprobe = 0, i = 0;
        for (;;) {
            const uint64_t idx = (hash + reprobe) & mask;
            reprobe += ++i;
            if (cells[idx].z == 0) {
                cells[idx].x = (uint32_t)key;
                cells[idx].y = (uint32_t)(key >> 32);
                cells[idx].z = targets[e];
                cells[idx].w = (uint32_t)e + 1u;
                if (targets[e] != 0) occ++;
                if (++size > nslots - 32) return kid_fail(KID_ERR_TABLE_FULL, "out of memory in table");
                break;
            }
        }
    }
    *n_occupied = occ;
    return KID_OK;
}

static int kid_db_build_common(const uint64_t *h_keys, const uint32_t *h_targets, const void *d_keys_in,
                               const void *d_targets_in, uint64_t n, const int32_t *parent, int32_t ntar, int k,
                               int log2_slots, int max_probes, uint32_t flags, int device, kid_db **out)
{
    if (!out) return kid_fail(KID_ERR_ARG, "out is null");
    *out = nullptr;
    if (!parent || ntar < 2) return kid_fail(KID_ERR_ARG, "parent is null or ntar < 2");
    if (k < 1 || k > 31) return kid_fail(KID_ERR_ARG, "k = %d outside [1,31]", k);
    if (log2_slots < 6 || log2_slots > 32) return kid_fail(KID_ERR_ARG, "log2_slots = %d outside [6,32]", log2_slots);
    if (max_probes < 0) return kid_fail(KID_ERR_ARG, "max_probes < 0");
    if (n > 0 && !((h_keys && h_targets) || (d_keys_in && d_targets_in))) return kid_fail(KID_ERR_ARG, "keys/targets null");
    if (n >= 0xFFFFFFFFull) return kid_fail(KID_ERR_ARG, "more than 2^32-2 entries");
    const uint64_t nslots = 1ULL << log2_slots;
    if (n > nslots - 32) return kid_fail(KID_ERR_TABLE_FULL, "out of memory in table");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;

    std::vector<int32_t> par, depth;
    int max_depth = 0;
    rc = kid_prepare_tree(parent, ntar, par, depth, max_depth);
    if (rc != KID_OK) return rc;
    if (h_targets)
        for (uint64_t i = 0; i < n; i++)
            if (h_targets[i] >= (uint32_t)ntar) return kid_fail(KID_ERR_TARGET, "targets[%llu] = %u >= ntar", (unsigned long long)i, h_targets[i]);

    KidDbPtr db = kid_db_new(device);
    const uint64_t table_bytes = nslots * sizeof(uint4);
    KID_HIP(db->table.alloc(table_bytes));
    // the per-sample seen-bitmap has one bit per ENTRY (its insertion ordinal, cell word 3), not per cell: a key's bit
    // is then the same in every table built from the same entries, whatever the cell placement -- what lets samples of
    // different GPUs (each with its own replica of the table) be OR-ed.  ord_target maps a bit back to its target.
    db->seen_bits = ((n + 127) / 128) * 128;
    if (db->seen_bits == 0) db->seen_bits = 128;
    KID_HIP(db->ord_target.alloc(db->seen_bits * 4));
    KID_HIP(hipMemset(db->ord_target.p, 0, db->seen_bits * 4));
    if (n > 0) {
        if (h_targets) KID_HIP(hipMemcpy(db->ord_target.p, h_targets, n * 4, hipMemcpyHostToDevice));
        else KID_HIP(hipMemcpy(db->ord_target.p, d_targets_in, n * 4, hipMemcpyDeviceToDevice));
    }
    KID_HIP(db->parent.alloc(sizeof(int32_t) * (size_t)ntar));
    KID_HIP(db->depth.alloc(sizeof(int32_t) * (size_t)ntar));
    KID_HIP(hipMemcpy(db->parent.p, par.data(), sizeof(int32_t) * (size_t)ntar, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(db->depth.p, depth.data(), sizeof(int32_t) * (size_t)ntar, hipMemcpyHostToDevice));
    const bool rows_ok = (max_depth <= 8 && ntar <= 65536);
    if (rows_ok) {
        std::vector<uint4> rows;
        kid_make_rows(par, depth, rows);
        KID_HIP(db->rows.alloc(sizeof(uint4) * (size_t)ntar));
        KID_HIP(hipMemcpy(db->rows.p, rows.data(), sizeof(uint4) * (size_t)ntar, hipMemcpyHostToDevice));
    }

    uint64_t n_occupied = 0;
    const bool host_build = (max_probes > 0) || (flags & KID_FLAG_HOST_BUILD);
    // minimizer-localised placement needs an unbounded probe loop (results must not depend on the
    // cell geometry) and k >= 24 (minimizers of k - 14 >= 10 bases)
    // (7 of 8 cells hold entries, and chains need free lines: at most 80 % of the cells may be taken)
    const uint32_t minloc = (!host_build && !(flags & KID_FLAG_REF_GEOMETRY) && k >= 24 && n <= (nslots / 10) * 8) ? 1u : 0u;
    const uint32_t line_bits = (uint32_t)log2_slots - 3u;
    const uint32_t line_shift = 32u - line_bits, line_mask = (uint32_t)((nslots >> 3) - 1);
    if (host_build) {
        std::vector<uint64_t> hk;
        std::vector<uint32_t> ht;
        if (!h_keys && n > 0) { // entries live on the device: fetch them
            hk.resize(n); ht.resize(n);
            KID_HIP(hipMemcpy(hk.data(), d_keys_in, n * 8, hipMemcpyDeviceToHost));
            KID_HIP(hipMemcpy(ht.data(), d_targets_in, n * 4, hipMemcpyDeviceToHost));
            h_keys = hk.data(); h_targets = ht.data();
            for (uint64_t i = 0; i < n; i++)
                if (h_targets[i] >= (uint32_t)ntar) return kid_fail(KID_ERR_TARGET, "targets[%llu] >= ntar", (unsigned long long)i);
        }
        struct Free { void operator()(uint4 *p) const { free(p); } };
        std::unique_ptr<uint4[], Free> cells((uint4 *)calloc(nslots, sizeof(uint4)));
        if (!cells) return kid_fail(KID_ERR_NOMEM, "host table of %llu bytes", (unsigned long long)table_bytes);
        rc = kid_host_build(h_keys, h_targets, n, log2_slots, cells.get(), &n_occupied);
        if (rc != KID_OK) return rc;
        KID_HIP(hipMemcpy(db->table.p, cells.get(), table_bytes, hipMemcpyHostToDevice));
    } else {
        KID_HIP(hipMemset(db->table.p, 0, table_bytes));
        if (n > 0) {
            KidDevBuf dk, d_occ;
            const uint64_t *dkc = (const uint64_t *)d_keys_in;
            const uint32_t *dtc = db->ord_target.as<uint32_t>();
            if (!dkc) {
                KID_HIP(dk.alloc(n * 8));
                KID_HIP(hipMemcpy(dk.p, h_keys, n * 8, hipMemcpyHostToDevice));
                dkc = dk.as<uint64_t>();
            }
            KID_HIP(d_occ.alloc(16));
            KID_HIP(hipMemset(d_occ.p, 0, 16));
            const int grid = kid_grid_for(n, 256, db->num_cu * 16);
            hipLaunchKernelGGL(kid_build_insert_kernel, dim3(grid), dim3(256), 0, 0, db->table.as<uint4>(), (uint32_t)(nslots - 1), dkc,
                               dtc, n, (uint32_t)ntar, d_occ.as<unsigned long long>(), k, minloc, line_shift, line_mask);
            hipLaunchKernelGGL(kid_build_firstwins_kernel, dim3(grid), dim3(256), 0, 0, db->table.as<uint4>(), (uint32_t)(nslots - 1),
                               dkc, dtc, n, k, minloc, line_shift, line_mask);
            KID_HIP(hipDeviceSynchronize());
            unsigned long long occ[2] = {0, 0};
            KID_HIP(hipMemcpy(occ, d_occ.p, 16, hipMemcpyDeviceToHost));
            if (occ[1] != 0) return kid_fail(KID_ERR_TARGET, "%llu targets >= ntar", occ[1]);
            n_occupied = occ[0];
        }
        if (minloc) { // the digest plane, from the finished headers (of an empty table too: all zero)
            const uint64_t n_lines = nslots >> 3;
            KID_HIP(db->digest.alloc(n_lines * sizeof(uint2)));
            hipLaunchKernelGGL(kid_build_digest_kernel, dim3(kid_grid_for(n_lines, KID_BUILD_BLOCK, db->num_cu * 16)), dim3(KID_BUILD_BLOCK), 0, 0,
                               db->table.as<uint4>(), n_lines, db->digest.as<uint2>());
            KID_HIP(hipDeviceSynchronize());
        }
    }

    db->d.table = db->table.as<uint4>();
    db->d.digest = db->digest.as<uint2>();
    db->d.nslots = nslots;
    db->d.slot_mask = (uint32_t)(nslots - 1);
    db->d.max_probes = (uint32_t)max_probes;
    db->d.k = k;
    db->d.u_is_t = (flags & KID_FLAG_U_IS_T) ? 1u : 0u;
    db->d.minloc = minloc;
    db->d.line_shift = line_shift;
    db->d.line_mask = line_mask;
    db->info.geometry = (int32_t)minloc;
    db->d.rows = db->rows.as<uint4>();
    db->d.parent = db->parent.as<int32_t>();
    db->d.depth = db->depth.as<int32_t>();
    db->d.ntar = ntar;
    db->info.ntar = ntar;
    db->info.k = k;
    db->info.log2_slots = log2_slots;
    db->info.max_probes = max_probes;
    db->info.flags = flags;
    db->info.device = device;
    db->info.tree_depth = max_depth;
    db->info.host_built = host_build ? 1 : 0;
    db->info.n_entries = n;
    db->info.n_occupied = n_occupied;
    db->info.table_bytes = table_bytes;
    *out = db.release();
    return KID_OK;
}

extern "C" int kid_db_build(const uint64_t *keys, const uint32_t *targets, uint64_t n, const int32_t *parent, int32_t ntar,
                            int k, int log2_slots, int max_probes, uint32_t flags, int device, kid_db **out)
{
    return kid_db_build_common(keys, targets, nullptr, nullptr, n, parent, ntar, k, log2_slots, max_probes, flags, device, out);
}

extern "C" int kid_db_build_device(const void *d_keys, const void *d_targets, uint64_t n, const int32_t *parent,
                                   int32_t ntar, int k, int log2_slots, int max_probes, uint32_t flags, int device,
                                   kid_db **out)
{
    return kid_db_build_common(nullptr, nullptr, d_keys, d_targets, n, parent, ntar, k, log2_slots, max_probes, flags, device, out);
}

// A replica of a database on another GPU (or on the same one): device-to-device copies of the table (16 GiB at bact10
// scale: over xGMI between peers), the taxonomy arrays and the entry -> target map.  Entry ordinals are part of the
// cells, so the replicas' samples share one seen-bitmap numbering (kid_sample_end_merged).
extern "C" int kid_db_replicate(const kid_db *src, int device, kid_db **out)
{
    if (!src || !out) return kid_fail(KID_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    KidDbPtr db = kid_db_new(device);
    const size_t nt = (size_t)src->info.ntar;
    auto copy = [&](KidDevBuf &dst, const KidDevBuf &from, size_t nbytes) -> hipError_t {
        hipError_t e = dst.alloc(nbytes);
        if (e != hipSuccess) return e;
        if (device == src->device) return hipMemcpy(dst.p, from.p, nbytes, hipMemcpyDeviceToDevice);
        return hipMemcpyPeer(dst.p, device, from.p, src->device, nbytes);
    };
    KID_HIP(copy(db->table, src->table, src->info.table_bytes));
    if (src->digest.p) KID_HIP(copy(db->digest, src->digest, src->info.table_bytes / 16));
    KID_HIP(copy(db->parent, src->parent, sizeof(int32_t) * nt));
    KID_HIP(copy(db->depth, src->depth, sizeof(int32_t) * nt));
    if (src->rows.p) KID_HIP(copy(db->rows, src->rows, sizeof(uint4) * nt));
    db->seen_bits = src->seen_bits;
    KID_HIP(copy(db->ord_target, src->ord_target, db->seen_bits * 4));
    KID_HIP(hipDeviceSynchronize());
    db->d = src->d;
    db->d.table = db->table.as<uint4>();
    db->d.digest = db->digest.as<uint2>();
    db->d.rows = db->rows.as<uint4>();
    db->d.parent = db->parent.as<int32_t>();
    db->d.depth = db->depth.as<int32_t>();
    db->info = src->info;
    db->info.device = device;
    *out = db.release();
    return KID_OK;
}

extern "C" int kid_db_get_info(const kid_db *db, kid_db_info *out)
{
    if (!db || !out) return kid_fail(KID_ERR_ARG, "null argument");
    *out = db->info;
    return KID_OK;
}

extern "C" void kid_db_destroy(kid_db *db)
{
    if (!db) return;
    hipSetDevice(db->device); // the owners' destructors free on the current device
    delete db;
}

extern "C" int kid_db_lookup(kid_db *db, const uint64_t *keys, uint64_t n, uint32_t *targets, uint32_t *probes)
{
    if (!db || (n && (!keys || !targets))) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    if (n == 0) return KID_OK;
    KidDevBuf dk, dt, dp;
    KID_HIP(dk.alloc(n * 8));
    KID_HIP(dt.alloc(n * 4));
    if (probes) KID_HIP(dp.alloc(n * 4));
    KID_HIP(hipMemcpy(dk.p, keys, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_lookup_kernel, dim3(kid_grid_for(n, 256, db->num_cu * 16)), dim3(256), 0, 0, db->d, dk.as<uint64_t>(), n,
                       dt.as<uint32_t>(), dp.as<uint32_t>());
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(targets, dt.p, n * 4, hipMemcpyDeviceToHost));
    if (probes) KID_HIP(hipMemcpy(probes, dp.p, n * 4, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_hash_keys(int device, const uint64_t *keys, uint64_t n, uint64_t *out)
{
    if (n && (!keys || !out)) return kid_fail(KID_ERR_ARG, "null argument");
    int rc = kid_use_device(device);
    if (rc != KID_OK) return rc;
    if (n == 0) return KID_OK;
    KidDevBuf dk, dout;
    KID_HIP(dk.alloc(n * 8));
    KID_HIP(dout.alloc(n * 8));
    KID_HIP(hipMemcpy(dk.p, keys, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_fmix_kernel, dim3(kid_grid_for(n, 256, 4096)), dim3(256), 0, 0, dk.as<uint64_t>(), n, dout.as<uint64_t>());
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_db_msca(kid_db *db, const int32_t *x, const int32_t *y, uint64_t n, int32_t *out)
{
    if (!db || (n && (!x || !y || !out))) return kid_fail(KID_ERR_ARG, "null argument");
    for (uint64_t i = 0; i < n; i++)
        if (x[i] < 0 || x[i] >= db->info.ntar || y[i] < 0 || y[i] >= db->info.ntar)
            return kid_fail(KID_ERR_TARGET, "pair %llu outside [0,ntar)", (unsigned long long)i);
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    if (n == 0) return KID_OK;
    KidDevBuf dx, dy, dout;
    KID_HIP(dx.alloc(n * 4));
    KID_HIP(dy.alloc(n * 4));
    KID_HIP(dout.alloc(n * 4));
    KID_HIP(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(dy.p, y, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_msca_kernel, dim3(kid_grid_for(n, 256, db->num_cu * 16)), dim3(256), 0, 0, db->d, dx.as<int32_t>(),
                       dy.as<int32_t>(), n, dout.as<int32_t>());
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return KID_OK;
}

extern "C" int kid_trim_batch(kid_db *db, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, int32_t *start,
                              int32_t *stop, uint8_t *keep)
{
    if (!db) return kid_fail(KID_ERR_ARG, "null db");
    if (n_reads == 0) return KID_OK;
    if (!quals || !offsets || !start || !stop || !keep) return kid_fail(KID_ERR_ARG, "null argument");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] < offsets[r] || offsets[r + 1] - offsets[r] > 0x7FFFFFFFull)
            return kid_fail(KID_ERR_ARG, "bad offsets at read %llu", (unsigned long long)r);
    int rc = kid_use_device(db->device);
    if (rc != KID_OK) return rc;
    const uint64_t base0 = offsets[0], nbytes = offsets[n_reads] - base0;
    KidDevBuf dq, dkeep, doff, ds, de;
    std::vector<uint64_t> rel;
    const uint64_t *off_src = kid_rebased_offsets(offsets, n_reads, rel);
    KID_HIP(dq.alloc(nbytes + 16));
    KID_HIP(doff.alloc((n_reads + 1) * 8));
    KID_HIP(ds.alloc(n_reads * 4));
    KID_HIP(de.alloc(n_reads * 4));
    KID_HIP(dkeep.alloc(n_reads));
    if (nbytes) KID_HIP(hipMemcpy(dq.p, quals + base0, nbytes, hipMemcpyHostToDevice));
    KID_HIP(hipMemcpy(doff.p, off_src, (n_reads + 1) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kid_trim_kernel, dim3(kid_grid_for(n_reads, 256, db->num_cu * 16)), dim3(256), 0, 0, dq.as<uint8_t>(),
                       doff.as<uint64_t>(), n_reads, db->info.k, ds.as<int32_t>(), de.as<int32_t>(), dkeep.as<uint8_t>());
    KID_HIP(hipDeviceSynchronize());
    KID_HIP(hipMemcpy(start, ds.p, n_reads * 4, hipMemcpyDeviceToHost));
    KID_HIP(hipMemcpy(stop, de.p, n_reads * 4, hipMemcpyDeviceToHost));
    KID_HIP(hipMemcpy(keep, dkeep.p, n_reads, hipMemcpyDeviceToHost));
    return KID_OK;
}
