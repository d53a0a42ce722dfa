// kid_probes.hip.h -- one lookup, one hash, one msca per thread: what the parity tests call.
#pragma once
#include "kid_table.hip.h"

// ------------------------------------------------------------------ unit probes (parity tests)
__global__ void kid_lookup_kernel(const KidDevDb db, const uint64_t *keys, uint64_t n, uint32_t *targets, uint32_t *probes)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t slot, np;
        targets[i] = kid_dev_lookup(db, keys[i], slot, np);
        if (probes) probes[i] = np;
    }
}

// Hashtable::integerHash (newkmer_10nx.cpp:189-197) as the device computes it
__global__ void kid_fmix_kernel(const uint64_t *keys, uint64_t n, uint64_t *out)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = kid_fmix64(keys[i]);
}

__global__ void kid_msca_kernel(const KidDevDb db, const int32_t *x, const int32_t *y, uint64_t n, int32_t *out)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = (uint32_t)x[i], c = (uint32_t)y[i];
        uint32_t r;
        if (db.rows) {
            uint4 ro;
            r = kid_msca_rows(a, db.rows[a], c, db.rows[c], ro);
        } else {
            r = kid_msca_climb(db, a, c);
        }
        out[i] = (int32_t)r;
    }
}
