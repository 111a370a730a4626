// The tiled all-pairs scan of the 3-D search kernels (k_chamfer_nn, k_knn: mesh3d.hip; k_ray_cast: raycast.hip; k_pm_points,
// k_pm_faces, k_pm_winding: point_mesh.hip; the key also in mesh_bvh.hip): every query sees ALL candidates.  Candidates stream
// through LDS in tiles between two barriers and every lane reads the same one (a broadcast); when the queries alone do not fill the
// GPU the candidate range is split over blockIdx.y, and the splits of a query merge in its 64-bit key.  Tile sizes, block sizes,
// queries per lane and unroll factors belong to the kernels.
#pragma once

#include "common.h"

// ---- the key ----------------------------------------------------------------------------------------------------------------------
// {bits of a float32 value, index}, value in the high word.  Every value that is put is >= 0 (a squared distance, a ray's t > t_min
// >= 0), so its bits order like the value and the 64-bit integers order like (value, index): atomicMin / atomicMax over a query's
// splits give what one sequential scan gives, whatever the order, and two calls give the same bits.
//   minimum: cleared to all ones (SCAN_KEY_NONE), equal values keep the smaller index, as a scan with a strict < does;
//   maximum: cleared to 0, equal values keep the larger index, as a scan with >= does.
#define SCAN_KEY_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ unsigned long long scan_key(float value, int index) {
    return ((unsigned long long)__float_as_uint(value) << 32) | (unsigned long long)(uint32_t)index;
}
__device__ __forceinline__ float scan_key_value(unsigned long long kv) { return __uint_as_float((uint32_t)(kv >> 32)); }
__device__ __forceinline__ int scan_key_index(unsigned long long kv) { return (int)(uint32_t)(kv & 0xFFFFFFFFull); }

// one split's result into the query's slot; a single split owns the slot and stores
__device__ __forceinline__ void scan_put_min(unsigned long long *slot, int splits, float value, int index) {
    if (splits == 1) *slot = scan_key(value, index);
    else atomicMin(slot, scan_key(value, index));
}
__device__ __forceinline__ void scan_put_max(unsigned long long *slot, int splits, float value, int index) {
    if (splits == 1) *slot = scan_key(value, index);
    else atomicMax(slot, scan_key(value, index));
}

// ---- the splits -------------------------------------------------------------------------------------------------------------------
// candidates [begin, end) of `count` that split blockIdx.y of `splits` takes, in whole tiles; a split behind the end gets nothing
__device__ __forceinline__ void scan_split_range(int count, int splits, int tile, int &begin, int &end) {
    const int chunk = ((count + splits - 1) / splits + tile - 1) / tile * tile;
    begin = (int)min((long long)blockIdx.y * chunk, (long long)count);
    end = min(count, begin + chunk);
}

// The host's split count: the caller's `requested` when > 0, else enough workgroups to fill the GPU (`fill`, with `qgroups` query
// workgroups over the whole launch) while every split still streams >= `min_tiles` tiles of its `candidates`; 1 .. 65535 (grid.y).
static inline int scan_splits(int requested, int qgroups, int candidates, int tile, int min_tiles, int fill) {
    if (requested > 0) return requested;
    int most = candidates / (min_tiles * tile);
    most = most > 65535 ? 65535 : most;
    const int wanted = ceil_div(fill, qgroups);
    most = most < wanted ? most : wanted;
    return most > 1 ? most : 1;
}

// ---- the tile loop ----------------------------------------------------------------------------------------------------------------
// stagings: what the whole workgroup does between the two barriers to put candidates c0 .. c0 + cnt - 1 into the tile

// (n, 3) floats -> one float4 per candidate; the tile is no larger than the workgroup
struct ScanStageXyz {
    const float *C;
    __device__ __forceinline__ void operator()(float4 *tile, int c0, int cnt) const {
        if ((int)threadIdx.x < cnt) {
            const float *p = C + 3 * (size_t)(c0 + threadIdx.x);
            tile[threadIdx.x] = make_float4(p[0], p[1], p[2], 0.f);
        }
    }
};

// three float4 rows per candidate (a face table {v0, e1, e2}), copied as they are by a workgroup of BLOCK threads
template <int BLOCK> struct ScanStageRows3 {
    const float4 *table;
    __device__ __forceinline__ void operator()(float4 *tile, int c0, int cnt) const {
        for (int i = threadIdx.x; i < 3 * cnt; i += BLOCK) tile[i] = table[3 * (size_t)c0 + i];
    }
};

// one tile staged between its two barriers (the first: every lane has finished reading the previous tile)
template <class Stage> __device__ __forceinline__ void scan_stage(float4 *tile, Stage stage, int c0, int cnt) {
    __syncthreads();
    stage(tile, c0, cnt);
    __syncthreads();
}

// body(c0, cnt) for every tile of [begin, end), the tile staged.  Block-uniform: every thread of the workgroup calls it with the
// same range.  (A kernel whose registers or instructions suffer from the body as a lambda writes this loop out around scan_stage and
// says so: profiles/scan_single_source.md.)
template <int TILE, class Stage, class Body>
__device__ __forceinline__ void scan_tiles(int begin, int end, float4 *tile, Stage stage, Body body) {
    for (int c0 = begin; c0 < end; c0 += TILE) {
        const int cnt = min(TILE, end - c0);
        scan_stage(tile, stage, c0, cnt);
        body(c0, cnt);
    }
}
