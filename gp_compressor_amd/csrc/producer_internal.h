// producer_internal.h -- what producer.hip (gpc_project_cloud) shares with registration.hip (gpc_registration_*): the voxel grid of a
// patch batch, the key arithmetic of its leaf table, and the batch object itself.
#pragma once

#include "gpc_internal.h"

// Both translation units are bit-exact against CPU restatements: floating-point contraction is off from here to their end, and
// every expression below is written in the association of oracle/gpc_oracle_producer.c.
#pragma clang fp contract(off)

struct PcGrid {
    double mn[3];       // minimum corner (the voxel grid's anchor)
    double res, radius, half;
    int kmax[3];        // largest voxel coordinate per axis
    int bx, by, bz;     // key = kz << (bx + by) | ky << bx | kx
    int sz;
};

__device__ static inline void pc_voxel(const PcGrid& g, float x, float y, float z, int k[3])
{
    k[0] = (int)floor(((double)x - g.mn[0]) / g.res);
    k[1] = (int)floor(((double)y - g.mn[1]) / g.res);
    k[2] = (int)floor(((double)z - g.mn[2]) / g.res);
}
__device__ static inline void pc_center(const PcGrid& g, const int k[3], double c[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = g.mn[a] + ((double)k[a] + 0.5) * g.res;
}
__host__ __device__ static inline uint64_t pc_pack(const PcGrid& g, int kx, int ky, int kz)
{
    return ((uint64_t)kz << (g.bx + g.by)) | ((uint64_t)ky << g.bx) | (uint64_t)kx;
}
__host__ __device__ static inline void pc_unpack(const PcGrid& g, uint64_t key, int k[3])
{
    k[0] = (int)(key & ((1ull << g.bx) - 1));
    k[1] = (int)((key >> g.bx) & ((1ull << g.by) - 1));
    k[2] = (int)(key >> (g.bx + g.by));
}

struct gpc_patches {
    gpc_ctx* ctx = nullptr;
    gpc_patches_view v{};       // device pointers into `block`
    void* block = nullptr;      // one allocation holds every array of the batch
    // the voxel table the batch was cut with (gpc_registration assigns a scan's points to the same leaves): leaf id = patch id
    PcGrid grid{};
    const uint64_t* leaf_key = nullptr;   // P sorted unique voxel keys, in `block`
    uint64_t serial = 0;        // gpc_child_register
};
