// What the translation units that work on a SmilHullGrid share (visual_hull.hip, distance_field.hip, hull_mesh.hip): the launch constants the
// grid's checks depend on, the device view of a grid, the workgroup scan and the scan of per-workgroup counts that the surface and the
// mesh share, the grid's validation, and the workspace layout that carries the caller's host tables.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"

#define HULL_THREADS 256
#define HULL_VOX 4       // voxels per thread of the carve, HULL_THREADS apart
#define HULL_SURF_VOX 4  // CONSECUTIVE voxels per thread of the surface kernels
#define HULL_MAX_VOXELS ((long long)1 << 40)

struct HullGridDev {
    const double *origin, *voxel;  // device copies of the caller's tables
    int n_origin, n_voxel;
    int Gx, Gy, Gz;
    long long vox;     // voxels of a frame
    long long chunks;  // workgroups of a frame
};

static inline long long hull_chunks(long long vox, int per_block) { return (vox + per_block - 1) / per_block; }

// The exclusive prefix of `mine` over the THREADS threads of the workgroup, and their sum in `total`: an inclusive scan of every
// wave, lane 63 stores its wave's sum, every thread adds the waves before it.  s_wave: THREADS / 64 entries of LDS, which a caller
// that comes back (the scan's rounds) may rewrite only behind a barrier of its own.
template <class T, int THREADS> __device__ __forceinline__ T block_scan_exclusive(T mine, T *s_wave, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan_inclusive(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        before += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    return before + incl - mine;
}

// (visual_hull.hip) Per-workgroup counts -> their exclusive prefixes, in place, for one or two jobs over the same n = N x chunks
// counts: offsets[f] = scale x the prefix of frame f's first workgroup, offsets[N] = scale x the total, which write_total_at_n
// also leaves in counts[n].  One workgroup of HULL_SCAN_THREADS per job.
#define HULL_SCAN_THREADS 1024
struct HullScanJob {
    long long *counts, *offsets;
    long long scale;
    int write_total_at_n;
};
int hull_scan(const HullScanJob *jobs, int n_jobs, long long n, long long chunks, int N, hipStream_t stream);

// what every check of a grid starts with: the grid is there, holds frames and voxels, at most 2^40 a frame (their number out)
static inline int check_hull_extent(const char *who, const SmilHullGrid *g, long long *vox) {
    SMIL_REQUIRE(g, "%s: null grid argument", who);
    SMIL_REQUIRE(g->N >= 1, "%s: N=%d frames", who, g->N);
    SMIL_REQUIRE(g->Gx >= 1 && g->Gy >= 1 && g->Gz >= 1, "%s: grid extent %d x %d x %d below 1", who, g->Gx, g->Gy, g->Gz);
    SMIL_REQUIRE((long long)g->Gx * g->Gy <= HULL_MAX_VOXELS / g->Gz, "%s: grid %d x %d x %d exceeds 2^40 voxels a frame", who, g->Gx, g->Gy, g->Gz);
    *vox = (long long)g->Gx * g->Gy * g->Gz;
    return SMIL_OK;
}
// the same conditions without a word (the *_workspace_bytes functions answer 0)
static inline bool hull_extent_ok(const SmilHullGrid *g) {
    return g && g->N >= 1 && g->Gx >= 1 && g->Gy >= 1 && g->Gz >= 1 && (long long)g->Gx * g->Gy <= HULL_MAX_VOXELS / g->Gz;
}

// the grid's sizes; `tables`: origin and voxel_size are read too
static inline int check_hull_grid(const char *who, const SmilHullGrid *g, bool tables, long long *vox_out) {
    if (int rc = check_hull_extent(who, g, vox_out)) return rc;
    // the grid of the launch with the fewest voxels per workgroup (HULL_VOX = HULL_SURF_VOX per thread)
    SMIL_REQUIRE(hull_chunks(*vox_out, HULL_VOX * HULL_THREADS) <= 0x7FFFFFFFLL / g->N, "%s: N=%d frames of %lld voxels exceed the grid", who, g->N,
                 *vox_out);
    // sum of i^2 over a frame stays below 2^63
    const double gmax = (double)std::max(g->Gx, std::max(g->Gy, g->Gz));
    SMIL_REQUIRE((double)*vox_out * gmax * gmax < 9.0e18, "%s: grid %d x %d x %d overflows the int64 index sums", who, g->Gx, g->Gy, g->Gz);
    if (!tables) return SMIL_OK;
    SMIL_REQUIRE(g->origin && g->voxel_size, "%s: null origin or voxel_size", who);
    SMIL_REQUIRE(g->n_origin == 1 || g->n_origin == g->N, "%s: origin has %d rows; expected 1 or N=%d", who, g->n_origin, g->N);
    SMIL_REQUIRE(g->n_voxel_size == 1 || g->n_voxel_size == g->N, "%s: voxel_size has %d rows; expected 1 or N=%d", who, g->n_voxel_size, g->N);
    for (int n = 0; n < g->n_voxel_size; ++n)
        SMIL_REQUIRE(g->voxel_size[n] > 0.0 && std::isfinite(g->voxel_size[n]), "%s: voxel_size[%d]=%g must be positive and finite", who, n,
                     g->voxel_size[n]);
    for (int n = 0; n < 3 * g->n_origin; ++n)
        SMIL_REQUIRE(std::isfinite(g->origin[n]), "%s: origin[%d][%d]=%g must be finite", who, n / 3, n % 3, g->origin[n]);
    return SMIL_OK;
}

// the caller's (host) tables uploaded behind `counts` entries of the workspace; null base: sizes only
struct HullWorkspace { long long *counts; double *origin, *voxel; size_t bytes; };
static inline HullWorkspace hull_layout(void *base, const SmilHullGrid *g, long long counts) {
    Workspace ws{(char *)base};
    HullWorkspace w;
    w.counts = ws.take<long long>((size_t)counts);
    w.origin = ws.take<double>(3 * (size_t)g->n_origin);
    w.voxel = ws.take<double>((size_t)g->n_voxel_size);
    w.bytes = ws.used;
    return w;
}
static inline int hull_upload(const HullWorkspace &w, const SmilHullGrid *g, long long vox, int per_block, HullGridDev *d, hipStream_t stream) {
    SMIL_HIP(hipMemcpyAsync(w.origin, g->origin, 3 * (size_t)g->n_origin * sizeof(double), hipMemcpyHostToDevice, stream));
    SMIL_HIP(hipMemcpyAsync(w.voxel, g->voxel_size, (size_t)g->n_voxel_size * sizeof(double), hipMemcpyHostToDevice, stream));
    *d = HullGridDev{w.origin, w.voxel, g->n_origin, g->n_voxel_size, g->Gx, g->Gy, g->Gz, vox, hull_chunks(vox, per_block)};
    return SMIL_OK;
}

