// The "spatial diameter" values of the SDF-guided registration term, by brute-force ray casting, for gfx950.
//
// Replaces (reference): fitter_3d/SDF_tests.py compute_ray_mesh_intersections_vectorized (:112-222), one Moeller-Trumbore test of a
// ray against every face written as ~30 torch ops, and the ray / sample loops of compute_sdf (:344-382) around it.
//
//  * k_ray_faces    thread per face: the face table {v0, e1 = v1 - v0, e2 = v2 - v0} as three float4, written once per call.  A face
//                   with a vertex index outside [0, V) becomes a point (e1 = e2 = 0: |a| = 0, never hit).
//  * k_ray_cast     lane = one ray; the rays of a sample sit in adjacent lanes.  Face tiles stream through LDS and every lane reads the
//                   same face (three ds_read_b128 broadcasts per face against ~45 VALU instructions per lane: the LDS is a quarter
//                   busy).  The lane keeps the LARGEST t over its hits and the face it belongs to - the reference takes torch.max of
//                   the distances, not the nearest hit.  When the rays do not fill the GPU the face range is split over workgroups;
//                   the splits merge in the ray's key, maximum flavour: every hit has t > t_min >= 0 (equal t: the larger face
//                   index, as the scan's >= gives).  The key, the split's range and count and the staging are scan.h's.
//  * k_ray_reduce   thread per sample, in ray order: the winning face's t once more in float64 (the float32 search decides WHICH face,
//                   its value is then the float64 formula's rounded to float32: the cancellation in s x e1 no longer shows in the
//                   result), the thresholds, the cap and the mean (a float64 sum, rounded once).
//
// No float atomics, no synchronisation: two calls on the same inputs give the same bits.  There is no BVH or grid: the exact maximum
// over ALL faces is what the reference computes.
#include "scan.h"

#define RC_BLOCK 256
#define RC_TILE 256   // faces staged in LDS per step (12 KB)
#define RC_EPS 1e-6f  // SDF_tests.py:156

struct RayArgs {
    const float *verts;    // (V, 3)
    const int *faces;      // (F, 3)
    const float *origins;  // (S, 3)
    const int *own_face;   // (S)
    const float *dirs;     // (S, R, 3)
    int V, F, S, R, splits, cap;
    float t_min, d_lo, d_hi;
    float4 *table;         // (F, 3) {v0, e1, e2}
    unsigned long long *key;  // (S, R) {bits of the largest t, its face}, 0: nothing hit
    float *ray_t;          // (S, R) or NULL
    float *diam;           // (S)
};

__global__ void __launch_bounds__(256) k_ray_faces(RayArgs a) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.F) return;
    const int i0 = a.faces[3 * (size_t)j], i1 = a.faces[3 * (size_t)j + 1], i2 = a.faces[3 * (size_t)j + 2];
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = v0, e2 = v0;
    if ((unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V) {
        const float *p0 = a.verts + 3 * (size_t)i0, *p1 = a.verts + 3 * (size_t)i1, *p2 = a.verts + 3 * (size_t)i2;
        v0 = make_float4(p0[0], p0[1], p0[2], 0.f);
        e1 = make_float4(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], 0.f);
        e2 = make_float4(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], 0.f);
    }
    a.table[3 * (size_t)j] = v0;
    a.table[3 * (size_t)j + 1] = e1;
    a.table[3 * (size_t)j + 2] = e2;
}

// 46 floating-point operations per (ray, face) as written: s 3, h 9, a 5, s.h 5, q 9, d.q 5, e2.q 5, 1/a 1, u v t 3, u + v 1.
__global__ void __launch_bounds__(RC_BLOCK) k_ray_cast(RayArgs a) {
#pragma clang fp contract(off)  // the products and sums below are rounded as written (u + v is not fused with v's product)
    __shared__ float4 tile[3 * RC_TILE];
    const int n_rays = a.S * a.R;
    const int r = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int rc = r < n_rays ? r : n_rays - 1;
    int f_begin, f_end;
    scan_split_range(a.F, a.splits, RC_TILE, f_begin, f_end);
    if (f_begin >= f_end) return;  // (block-uniform)
    const int s_id = rc / a.R;
    const float ox = a.origins[3 * (size_t)s_id], oy = a.origins[3 * (size_t)s_id + 1], oz = a.origins[3 * (size_t)s_id + 2];
    const float dx = a.dirs[3 * (size_t)rc], dy = a.dirs[3 * (size_t)rc + 1], dz = a.dirs[3 * (size_t)rc + 2];
    const int own = a.own_face[s_id];
    const float t_min = a.t_min;
    float best = 0.f;
    int best_face = 0;
    for (int f0 = f_begin; f0 < f_end; f0 += RC_TILE) {  // (scan_tiles written out: as a lambda the body costs 24 % of the time)
        const int cnt = min(RC_TILE, f_end - f0);
        scan_stage(tile, ScanStageRows3<RC_BLOCK>{a.table}, f0, cnt);
        const int skip = own - f0;  // the sample's own face within this tile, or out of range
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const float4 v0 = tile[3 * j], e1 = tile[3 * j + 1], e2 = tile[3 * j + 2];
            const float hx = fmaf(dy, e2.z, -(dz * e2.y)), hy = fmaf(dz, e2.x, -(dx * e2.z)), hz = fmaf(dx, e2.y, -(dy * e2.x));
            const float det = fmaf(e1.z, hz, fmaf(e1.y, hy, e1.x * hx));
            const float sx = ox - v0.x, sy = oy - v0.y, sz = oz - v0.z;
            const float sh = fmaf(sz, hz, fmaf(sy, hy, sx * hx));
            const float qx = fmaf(sy, e1.z, -(sz * e1.y)), qy = fmaf(sz, e1.x, -(sx * e1.z)), qz = fmaf(sx, e1.y, -(sy * e1.x));
            const float dq = fmaf(dz, qz, fmaf(dy, qy, dx * qx));
            const float eq = fmaf(e2.z, qz, fmaf(e2.y, qy, e2.x * qx));
            const float f = 1.0f / det;
            const float u = f * sh, v = f * dq, t = f * eq;
            const bool hit = (j != skip) & (fabsf(det) > RC_EPS) & (u >= 0.0f) & (u <= 1.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t > t_min);
            const bool take = hit & (t >= best);
            best = take ? t : best;
            best_face = take ? f0 + j : best_face;
        }
    }
    if (r < n_rays && best > 0.f) scan_put_max(&a.key[r], a.splits, best, best_face);
}

__global__ void __launch_bounds__(256) k_ray_reduce(RayArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const double o[3] = {a.origins[3 * (size_t)s], a.origins[3 * (size_t)s + 1], a.origins[3 * (size_t)s + 2]};
    double sum = 0.0;
    int taken = 0;
    for (int k = 0; k < a.R; ++k) {
        const size_t r = (size_t)s * a.R + k;
        const unsigned long long kv = a.key[r];
        float t = -1.0f;
        if (kv) {  // (a key's face passed k_ray_faces' index check: a face with a bad index is never hit)
            const int *fi = a.faces + 3 * (size_t)scan_key_index(kv);
            const float *p0 = a.verts + 3 * (size_t)fi[0], *p1 = a.verts + 3 * (size_t)fi[1], *p2 = a.verts + 3 * (size_t)fi[2];
            const double d[3] = {a.dirs[3 * r], a.dirs[3 * r + 1], a.dirs[3 * r + 2]};
            const double e1[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
            const double e2[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
            const double sv[3] = {o[0] - p0[0], o[1] - p0[1], o[2] - p0[2]};
            const double h[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
            const double q[3] = {sv[1] * e1[2] - sv[2] * e1[1], sv[2] * e1[0] - sv[0] * e1[2], sv[0] * e1[1] - sv[1] * e1[0]};
            const double det = e1[0] * h[0] + e1[1] * h[1] + e1[2] * h[2];
            t = (float)((1.0 / det) * (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]));
        }
        if (a.ray_t) a.ray_t[r] = t;
        if (kv && taken < a.cap && a.d_lo < t && t < a.d_hi) {  // SDF_tests.py:355-376: in ray order until `cap` valid rays are taken
            sum += (double)t;
            ++taken;
        }
    }
    a.diam[s] = taken ? (float)(sum / (double)taken) : a.d_lo;
}

static size_t ray_layout(int F, int S, int R, char *base, RayArgs &a) {
    Workspace w{base};
    a.table = w.take<float4>((size_t)F * 3);
    a.key = w.take<unsigned long long>((size_t)S * R);
    return w.used;
}

static bool ray_sizes_ok(int64_t V, int64_t F, int64_t S, int64_t R) {
    return V > 0 && F > 0 && S > 0 && R > 0 && S * R <= 0x7FFFFFFF - RC_BLOCK && F <= 0x7FFFFFFF - RC_TILE;
}

extern "C" size_t smil_ray_diameters_workspace_bytes(int32_t F, int32_t S, int32_t R) {
    RayArgs a;
    return ray_sizes_ok(1, F, S, R) ? ray_layout(F, S, R, nullptr, a) : 0;
}

extern "C" int smil_ray_diameters(const float *verts, int32_t V, const int32_t *faces, int32_t F, const float *origins, const int32_t *own_face,
                                  const float *dirs, int32_t S, int32_t R, float t_min, float d_lo, float d_hi, int32_t cap, float *ray_t,
                                  float *diam, void *workspace, void *stream_) {
    SMIL_REQUIRE(verts && faces && origins && own_face && dirs && diam && workspace, "smil_ray_diameters: null argument");
    SMIL_REQUIRE(ray_sizes_ok(V, F, S, R), "smil_ray_diameters: bad sizes V=%d F=%d S=%d R=%d", V, F, S, R);
    SMIL_REQUIRE(t_min >= 0.f, "smil_ray_diameters: t_min=%g must be >= 0 (the splits merge on the bits of t)", (double)t_min);
    SMIL_REQUIRE(cap >= 1, "smil_ray_diameters: cap=%d must be >= 1", cap);
    hipStream_t stream = (hipStream_t)stream_;
    RayArgs a;
    ray_layout(F, S, R, (char *)workspace, a);
    a.verts = verts; a.faces = (const int *)faces; a.origins = origins; a.own_face = (const int *)own_face; a.dirs = dirs;
    a.V = V; a.F = F; a.S = S; a.R = R; a.cap = cap;
    a.t_min = t_min; a.d_lo = d_lo; a.d_hi = d_hi;
    a.ray_t = ray_t; a.diam = diam;
    const int rblocks = ceil_div(S * R, RC_BLOCK);
    a.splits = scan_splits(0, rblocks, F, RC_TILE, 4, 2048);  // >= 2048 workgroups while every split still streams >= 4 tiles
    SMIL_HIP(hipMemsetAsync(a.key, 0, (size_t)S * R * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_ray_faces, dim3(ceil_div(F, 256)), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ray_cast, dim3(rblocks, a.splits), dim3(RC_BLOCK), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ray_reduce, dim3(ceil_div(S, 256)), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
