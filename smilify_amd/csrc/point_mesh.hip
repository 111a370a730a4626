// Exact distances between point clouds and triangle meshes, both directions, with gradients, for gfx950.
//
// An extension (the reference never asks "how far is this point from this surface"): pytorch3d names the operation
// loss.point_mesh_face_distance; the definition here is the true Euclidean distance to the CLOSED triangle, degenerate faces included
// (point_tri.h), without pytorch3d's min_triangle_area rule.
//
//  * k_pm_extent    the largest finite |coordinate| of every mesh's face vertices and points, as the bits of a float (atomicMax).  The
//                   search runs in the mesh's FRAME: every coordinate times 2^-ex, the power of two that brings that largest value
//                   below 1.  Scaling by a power of two is exact, so the float32 search sees the same roundings whatever the data's
//                   unit, its degree-4 products (va, vb, vc of point_tri.h) neither overflow nor underflow for data of any extent, and
//                   scaling all inputs by a power of two changes no selection.
//  * k_pm_table     thread per face: {v0, e1 = v1 - v0, e2 = v2 - v0} in the frame as three float4, written once per call.  A face
//                   with a non-finite vertex or a vertex index outside [0, n_verts) gets v0 = NaN: its distance is NaN, which is never
//                   < the running minimum, so it never wins.
//  * k_pm_points    points -> faces.  lane = one point; face tiles stream through LDS and every lane reads the same face (three
//                   ds_read_b128 broadcasts against ~110 VALU instructions per point).  Running minimum of the float32 squared
//                   distance with a strict <.  The face range may be split over blockIdx.y; the splits merge in the point's key,
//                   minimum flavour: a tie goes to the smaller face index, as one sequential scan gives.  The key, the split's
//                   range and count and the staging between two barriers are scan.h's, here and in the next two.
//  * k_pm_faces     faces -> points: the same device function with the roles swapped.  lane = one face (its table entry in registers),
//                   the cloud's points stream through LDS in the frame, the point range may be split, the same merge.
//  * k_pm_winding   the generalised winding number of every point (Jacobson et al. 2013): the sum over ALL faces of the signed solid
//                   angle Omega_f / (4 pi), by van Oosterom & Strackee's formula in float32 in the frame.  k_pm_points' prologue and
//                   loop (pm_points_over_faces) around another per-face body.  A pair whose det is +-0 adds exactly 0 (a degenerate
//                   face, a point in the face's plane or on a vertex).  Every pair's value (|.| <= 0.5) goes to int64 fixed point
//                   whose unit follows the mesh's face count and is added as an integer, in the lane and, when the faces are split,
//                   with one 64-bit atomicAdd per point and split: two calls, every split count and every order of the faces give
//                   the same bits.  k_pm_winding_finish converts once to float32; a padded or unusable point gets NaN.
//  * k_pm_finish    thread per query (point or face): the winner's closest point once more in float64 from the float32 inputs (the
//                   float32 search decides WHICH, the value is the float64 formula's, rounded once), the barycentrics and the index.
//                   No winner (a non-finite or padded point, a mesh without a face that can win, an empty cloud): +inf, -1, 0.
//  * k_pm_bwd_*     the gradient of records (query, index) with an upstream gradient g per record: with c the closest point (float64,
//                   recomputed at the recorded pair) and e = p - c, d/dp = 2 g e and d/dv_k = -2 g b_k e.  The side that owns the
//                   record (the point, points -> faces) writes directly; vertices (shared by faces, faces hit by many points) and the
//                   points picked by many faces are summed as int64 fixed point whose unit follows the mesh's largest addend and its
//                   record count (common.h "order-independent scatter sums"): no float atomics, two calls give equal bits, a
//                   permutation of the points leaves the vertex gradients bit-identical.
//
// These kernels use no BVH, grid or cull: the exact minimum over ALL faces is the contract, as in raycast.hip.
// mesh_bvh.hip finds the same winner through a hierarchy (section 4.22) between this file's pm_prepare() and pm_finish().
#include "point_mesh.h"

#define PM_BLOCK 256
#define PM_TILE 128  // faces (48 B) or points (16 B) staged in LDS per step

// (every lane of every wave reaches fix_record_max)
__global__ void __launch_bounds__(256) k_pm_extent(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    float big = 0.f;
    int id[3];
    if (t < m.F && pm_face_ids(a, (size_t)m.f0 + t, id)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *v = a.verts + 3 * (size_t)id[k];
            big = fmaxf(big, fmaxf(pm_finite_abs(v[0]), fmaxf(pm_finite_abs(v[1]), pm_finite_abs(v[2]))));
        }
    }
    if (t < m.len) {
        const float *p = a.points + ((size_t)n * a.P + t) * 3;
        big = fmaxf(big, fmaxf(pm_finite_abs(p[0]), fmaxf(pm_finite_abs(p[1]), pm_finite_abs(p[2]))));
    }
    fix_record_max(&a.ext[n], big);
}

__global__ void __launch_bounds__(256) k_pm_table(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    if (t >= m.F) return;
    const size_t j = (size_t)m.f0 + t;
    const int sh = pm_frame(a, n);
    const float nan = __builtin_nanf("");
    float4 v0 = make_float4(nan, nan, nan, 0.f), e1 = make_float4(0.f, 0.f, 0.f, 0.f), e2 = e1;
    float c[9];
    if (pm_face_coords(a, j, c)) {  // (the .w slots: n = e1 x e2 for k_pm_winding; the distance kernels do not read them)
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] = ldexpf(c[k], sh);
        const float ux = c[3] - c[0], uy = c[4] - c[1], uz = c[5] - c[2], vx = c[6] - c[0], vy = c[7] - c[1], vz = c[8] - c[2];
        v0 = make_float4(c[0], c[1], c[2], uy * vz - uz * vy);
        e1 = make_float4(ux, uy, uz, uz * vx - ux * vz);
        e2 = make_float4(vx, vy, vz, ux * vy - uy * vx);
    }
    a.table[3 * j] = v0;
    a.table[3 * j + 1] = e1;
    a.table[3 * j + 2] = e2;
}

// What k_pm_points and k_pm_winding share.  Lane = point q of mesh n's cloud, in the frame; face(px, py, pz, f, v0, e1, e2) for
// every face f of the split blockIdx.y, from the tile.  `at`: the point's row in the (N, P) arrays; false: the lane has no point
// (a lane behind the cloud's end repeats its last point and writes nothing), or the workgroup has no points or no faces.
template <class Face>
__device__ __forceinline__ bool pm_points_over_faces(const PmArgs &a, int n, const PmMesh &m, float4 *tile, size_t &at, Face face) {
    const int q = blockIdx.x * PM_BLOCK + threadIdx.x;
    if ((int)(blockIdx.x * PM_BLOCK) >= m.len) return false;  // (block-uniform, as the next)
    int f_begin, f_end;
    scan_split_range(m.F, a.splits, PM_TILE, f_begin, f_end);
    if (f_begin >= f_end) return false;
    const int sh = pm_frame(a, n);
    const float *Q = a.points + (size_t)n * a.P * 3;
    float px, py, pz;
    pm_load_point(Q + 3 * (size_t)min(q, m.len - 1), sh, px, py, pz);
    for (int f0 = f_begin; f0 < f_end; f0 += PM_TILE) {  // (scan_tiles written out: one lambda inside another costs 0.3 % and 3.5 %)
        const int cnt = min(PM_TILE, f_end - f0);
        scan_stage(tile, ScanStageRows3<PM_BLOCK>{a.table + 3 * (size_t)m.f0}, f0, cnt);
        for (int j = 0; j < cnt; ++j) face(px, py, pz, f0 + j, tile[3 * j], tile[3 * j + 1], tile[3 * j + 2]);
    }
    at = (size_t)n * a.P + q;
    return q < m.len;
}

__global__ void __launch_bounds__(PM_BLOCK) k_pm_points(PmArgs a) {
    __shared__ float4 tile[3 * PM_TILE];
    const int n = blockIdx.z;
    const PmMesh m = pm_mesh(a, n);
    float best = __builtin_inff();
    int bi = 0x7FFFFFFF;
    size_t at;
    const auto face = [&](float px, float py, float pz, int f, const float4 &v0, const float4 &e1, const float4 &e2) {
        const TriPoint<float> r = closest_on_triangle<float>(px - v0.x, py - v0.y, pz - v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
        const bool take = r.dist2 < best;
        best = take ? r.dist2 : best;
        bi = take ? f : bi;
    };
    // (+inf: nothing won in this split)
    if (pm_points_over_faces(a, n, m, tile, at, face) && best < __builtin_inff()) scan_put_min(&a.key[at], a.splits, best, bi);
}

__global__ void __launch_bounds__(PM_BLOCK) k_pm_faces(PmArgs a) {
    __shared__ float4 tile[PM_TILE];
    const int n = blockIdx.z;
    const PmMesh m = pm_mesh(a, n);
    const int t = blockIdx.x * PM_BLOCK + threadIdx.x;
    if ((int)(blockIdx.x * PM_BLOCK) >= m.F) return;  // (block-uniform, as the next)
    int p_begin, p_end;
    scan_split_range(m.len, a.splits, PM_TILE, p_begin, p_end);
    if (p_begin >= p_end) return;
    const int sh = pm_frame(a, n);
    const size_t j = (size_t)m.f0 + min(t, m.F - 1);
    const float4 v0 = a.table[3 * j], e1 = a.table[3 * j + 1], e2 = a.table[3 * j + 2];
    const float *Q = a.points + (size_t)n * a.P * 3;
    float best = __builtin_inff();
    int bi = 0x7FFFFFFF;
    const auto stage = [&](float4 *tile, int p0, int cnt) {  // ScanStageXyz through pm_load_point: the points in the frame
        if ((int)threadIdx.x < cnt) {
            float x, y, z;
            pm_load_point(Q + 3 * (size_t)(p0 + threadIdx.x), sh, x, y, z);
            tile[threadIdx.x] = make_float4(x, y, z, 0.f);
        }
    };
    for (int p0 = p_begin; p0 < p_end; p0 += PM_TILE) {  // (scan_tiles written out: as a lambda the body costs 11 % of the time)
        const int cnt = min(PM_TILE, p_end - p0);
        scan_stage(tile, stage, p0, cnt);
#pragma unroll 2
        for (int i = 0; i < cnt; ++i) {
            const float4 p = tile[i];
            const TriPoint<float> r = closest_on_triangle<float>(p.x - v0.x, p.y - v0.y, p.z - v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
            const bool take = r.dist2 < best;
            best = take ? r.dist2 : best;
            bi = take ? p0 + i : bi;
        }
    }
    if (t < m.F && best < __builtin_inff()) scan_put_min(&a.key[(size_t)m.f0 + t], a.splits, best, bi);  // (+inf: as in k_pm_points)
}

// The closest point of packed face j to point p of mesh n's cloud in float64, from the float32 inputs.  false: the pair does not
// exist, or one of its coordinates is not usable.
__device__ __forceinline__ bool pm_pair64(const PmArgs &a, int n, const PmMesh &m, int face, int point, TriPoint<double> &r, double (&e)[3],
                                          int (&id)[3]) {
    if (face < 0 || face >= m.F || point < 0 || point >= m.len) return false;
    if (!pm_face_ids(a, (size_t)m.f0 + face, id)) return false;
    const float *p = a.points + ((size_t)n * a.P + point) * 3;
    const float *v0 = a.verts + 3 * (size_t)id[0], *v1 = a.verts + 3 * (size_t)id[1], *v2 = a.verts + 3 * (size_t)id[2];
    bool usable = pm_usable3(p);  // (the search never pairs these, a hand-made record of the backward may)
    usable &= pm_usable3(v0); usable &= pm_usable3(v1); usable &= pm_usable3(v2);
    if (!usable) return false;
    const double e1[3] = {(double)v1[0] - v0[0], (double)v1[1] - v0[1], (double)v1[2] - v0[2]};
    const double e2[3] = {(double)v2[0] - v0[0], (double)v2[1] - v0[1], (double)v2[2] - v0[2]};
    const double ap[3] = {(double)p[0] - v0[0], (double)p[1] - v0[1], (double)p[2] - v0[2]};
    r = closest_on_triangle<double>(ap[0], ap[1], ap[2], e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = ap[k] - r.v * e1[k] - r.w * e2[k];
    return true;
}

// query t of mesh n is point t (a.by_face == 0) or face t; `at` its row in the outputs and keys, or false when there is no such query
__device__ __forceinline__ bool pm_query(const PmArgs &a, int n, const PmMesh &m, int t, size_t &at) {
    at = a.by_face ? (size_t)m.f0 + t : (size_t)n * a.P + t;
    return t < (a.by_face ? m.F : a.P);
}

__global__ void __launch_bounds__(256) k_pm_finish(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    size_t at;
    if (!pm_query(a, n, m, t, at)) return;
    const unsigned long long kv = a.key[at];
    const int other = scan_key_index(kv);
    TriPoint<double> r;
    double e[3];
    int id[3];
    const bool none = kv == SCAN_KEY_NONE || !pm_pair64(a, n, m, a.by_face ? t : other, a.by_face ? other : t, r, e, id);
    a.dist2[at] = none ? __builtin_inff() : (float)r.dist2;
    a.idx[at] = none ? -1 : other;
    a.bary[3 * at] = none ? 0.f : (float)r.b0;
    a.bary[3 * at + 1] = none ? 0.f : (float)r.v;
    a.bary[3 * at + 2] = none ? 0.f : (float)r.w;
}

// ---- winding numbers ------------------------------------------------------------------------------------------------------------
// Omega / (4 pi) of one face seen from p, everything in the frame: with a = v0 - p, b = a + e1, c = a + e2,
// tan(Omega / 2) = a . (e1 x e2) / (|a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|) (van Oosterom & Strackee 1983).  Positive when the
// face's normal e1 x e2 points away from p.  det == +-0 (and a NaN: an unusable face or point): exactly 0, so nothing hangs on the
// sign of a zero.
__device__ __forceinline__ float pm_face_angle(float px, float py, float pz, const float4 &v0, const float4 &e1, const float4 &e2) {
    const float ax = v0.x - px, ay = v0.y - py, az = v0.z - pz;
    const float bx = ax + e1.x, by = ay + e1.y, bz = az + e1.z;
    const float cx = ax + e2.x, cy = ay + e2.y, cz = az + e2.z;
    const float det = ax * v0.w + ay * e1.w + az * e2.w;
    const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
    const float ab = ax * bx + ay * by + az * bz, ac = ax * cx + ay * cy + az * cz, bc = bx * cx + by * cy + bz * cz;
    const float den = la * lb * lc + ab * lc + ac * lb + bc * la;
    return fabsf(det) > 0.f ? atan2f(det, den) * 0.15915494309189535f : 0.f;  // 1 / (2 pi)
}

// Unit exponent of mesh n's winding sums: |addend| <= 0.5 < 2^0, one addend per face.
__device__ __forceinline__ int pm_winding_fix(const PmMesh &m) { return fix_unit_exp(0, max(m.F, 1)); }

__global__ void __launch_bounds__(PM_BLOCK) k_pm_winding(PmArgs a) {
    __shared__ float4 tile[3 * PM_TILE];
    const int n = blockIdx.z;
    const PmMesh m = pm_mesh(a, n);
    const int fix = pm_winding_fix(m);
    long long sum = 0;
    size_t at;
    const auto face = [&](float px, float py, float pz, int, const float4 &v0, const float4 &e1, const float4 &e2) {
        sum += __double2ll_rn(ldexp((double)pm_face_angle(px, py, pz, v0, e1, e2), fix));
    };
    if (pm_points_over_faces(a, n, m, tile, at, face)) atomicAdd((unsigned long long *)&a.acc_p[at], (unsigned long long)sum);
}

__global__ void __launch_bounds__(256) k_pm_winding_finish(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.P) return;
    const PmMesh m = pm_mesh(a, n);
    const size_t at = (size_t)n * a.P + t;
    const bool usable = t < m.len && pm_usable3(a.points + 3 * at);
    a.winding[at] = usable ? fix_read(a.acc_p[at], pm_winding_fix(m)) : __builtin_nanf("");
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// record t of mesh n: the pair, its barycentrics and the point's gradient 2 g e (float64); false: the record contributes nothing
__device__ __forceinline__ bool pm_record(const PmArgs &a, int n, const PmMesh &m, int t, size_t &at, int &point, double (&b)[3], double (&ge)[3],
                                          int (&id)[3]) {
    if (!pm_query(a, n, m, t, at)) return false;
    const int other = a.idx[at];
    point = a.by_face ? other : t;
    TriPoint<double> r;
    double e[3];
    if (!pm_pair64(a, n, m, a.by_face ? t : other, point, r, e, id)) return false;
    const double g2 = 2.0 * (double)a.g[at];
    b[0] = r.b0; b[1] = r.v; b[2] = r.w;
#pragma unroll
    for (int k = 0; k < 3; ++k) ge[k] = g2 * e[k];
    return true;
}

// Unit exponent of mesh n's sums: every addend is a component of 2 g e times a barycentric <= 1, and at most three addends per record
// (a face may name one vertex three times) of at most max(P, F_n) records meet in one element.
__device__ __forceinline__ int pm_fix_exp(const PmArgs &a, int n, const PmMesh &m) {
    return fix_unit_exp(fix_max_exp(a.dmax[n]), 3ll * max(a.by_face ? m.F : a.P, 1) + 1);
}

__global__ void __launch_bounds__(256) k_pm_bwd_max(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    size_t at;
    int point, id[3];
    double b[3], ge[3];
    float big = 0.f;
    if (pm_record(a, n, m, t, at, point, b, ge, id))
        big = fmaxf(pm_finite_abs((float)ge[0]), fmaxf(pm_finite_abs((float)ge[1]), pm_finite_abs((float)ge[2])));
    fix_record_max(&a.dmax[n], big);
}

__global__ void __launch_bounds__(256) k_pm_bwd_add(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    size_t at;
    int point, id[3];
    double b[3], ge[3];
    const bool ok = pm_record(a, n, m, t, at, point, b, ge, id);
    if (!a.by_face && t < a.P) {  // the point owns its record
        float *d = a.d_points + ((size_t)n * a.P + t) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = ok ? (float)ge[k] : 0.f;
    }
    if (!ok) return;
    const int fix = pm_fix_exp(a, n, m);
    if (a.by_face) {
        long long *acc = a.acc_p + ((size_t)n * a.P + point) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(&acc[k], ge[k], fix);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long *acc = a.acc_v + 3 * (size_t)id[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(&acc[k], -b[c] * ge[k], fix);
    }
}

// thread t of mesh n: vertex t of the mesh, and (faces -> points) point t of its cloud
__global__ void __launch_bounds__(256) k_pm_bwd_out(PmArgs a) {
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    const int fix = pm_fix_exp(a, n, m);
    const int v0 = min(max(a.vert_off[n], 0), a.n_verts), v1 = min(max(a.vert_off[n + 1], v0), a.n_verts);
    if (t < v1 - v0) {
        const size_t v = (size_t)v0 + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.d_verts[3 * v + k] = fix_read(a.acc_v[3 * v + k], fix);
    }
    if (a.by_face && t < a.P) {
        const size_t p = (size_t)n * a.P + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.d_points[3 * p + k] = fix_read(a.acc_p[3 * p + k], fix);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
extern "C" size_t smil_point_mesh_workspace_bytes(int32_t N, int32_t F_total, int32_t P, int32_t n_verts) {
    PmArgs a;
    return pm_sizes_ok(N, F_total, P, n_verts) ? pm_layout(N, F_total, P, n_verts, nullptr, a) : 0;
}

// splits of `cols` candidates for `qblocks` workgroups of queries per mesh: the caller's, or >= 2048 workgroups while every split
// still streams >= 2 tiles
static int pm_splits(int32_t splits, int qblocks, int cols, int N) { return scan_splits(splits, qblocks * N, cols, PM_TILE, 2, 2048); }

int pm_prepare(PmArgs &a, int max_faces, size_t n_keys, hipStream_t stream) {
    if (n_keys) SMIL_HIP(hipMemsetAsync(a.key, 0xFF, n_keys * sizeof(unsigned long long), stream));
    SMIL_HIP(hipMemsetAsync(a.ext, 0, (size_t)a.N * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_pm_extent, dim3(ceil_div(std::max(max_faces, a.P), 256), a.N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pm_table, dim3(ceil_div(max_faces, 256), a.N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

int pm_finish(PmArgs &a, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(k_pm_finish, dim3(ceil_div(rows, 256), a.N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// the forward of either direction: `rows` queries and `cols` candidates per mesh at most
static int pm_forward(PmArgs &a, int max_faces, int32_t splits, hipStream_t stream) {
    const int rows = a.by_face ? max_faces : a.P, cols = a.by_face ? a.P : max_faces;
    const size_t n_keys = a.by_face ? (size_t)a.F_total : (size_t)a.N * a.P;
    const int qblocks = ceil_div(rows, PM_BLOCK);
    a.splits = pm_splits(splits, qblocks, cols, a.N);
    int rc = pm_prepare(a, max_faces, n_keys, stream);
    if (rc != SMIL_OK) return rc;
    const dim3 grid(qblocks, a.splits, a.N);
    if (a.by_face) hipLaunchKernelGGL(k_pm_faces, grid, dim3(PM_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_pm_points, grid, dim3(PM_BLOCK), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return pm_finish(a, rows, stream);
}

extern "C" int smil_point_face_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                        int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths,
                                        int32_t splits, float *dist2, int32_t *face, float *bary, void *workspace, void *stream) {
    PmArgs a;
    const int rc = pm_fill(a, "smil_point_face_distance", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(dist2 && face && bary, "smil_point_face_distance: null output");
    SMIL_REQUIRE(splits >= 0 && splits <= 65535, "smil_point_face_distance: splits=%d outside 0 .. 65535", splits);
    a.dist2 = dist2; a.idx = (int *)face; a.bary = bary; a.by_face = 0;
    return pm_forward(a, max_faces, splits, (hipStream_t)stream);
}

extern "C" int smil_face_point_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                        int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths,
                                        int32_t splits, float *dist2, int32_t *point, float *bary, void *workspace, void *stream) {
    PmArgs a;
    const int rc = pm_fill(a, "smil_face_point_distance", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(dist2 && point && bary, "smil_face_point_distance: null output");
    SMIL_REQUIRE(splits >= 0 && splits <= 65535, "smil_face_point_distance: splits=%d outside 0 .. 65535", splits);
    a.dist2 = dist2; a.idx = (int *)point; a.bary = bary; a.by_face = 1;
    return pm_forward(a, max_faces, splits, (hipStream_t)stream);
}

extern "C" int smil_point_mesh_winding(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                       int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths,
                                       int32_t splits, float *winding, void *workspace, void *stream_) {
    PmArgs a;
    const int rc = pm_fill(a, "smil_point_mesh_winding", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(winding, "smil_point_mesh_winding: null output");
    SMIL_REQUIRE(splits >= 0 && splits <= 65535, "smil_point_mesh_winding: splits=%d outside 0 .. 65535", splits);
    hipStream_t stream = (hipStream_t)stream_;
    a.winding = winding;
    const int qblocks = ceil_div(P, PM_BLOCK);
    a.splits = pm_splits(splits, qblocks, max_faces, N);
    SMIL_HIP(hipMemsetAsync(a.acc_p, 0, (size_t)N * P * sizeof(long long), stream));
    const int rc2 = pm_prepare(a, max_faces, 0, stream);  // (no keys: the splits meet in acc_p)
    if (rc2 != SMIL_OK) return rc2;
    hipLaunchKernelGGL(k_pm_winding, dim3(qblocks, a.splits, N), dim3(PM_BLOCK), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pm_winding_finish, dim3(ceil_div(P, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_point_mesh_backward(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off,
                                        const int32_t *vert_off, int32_t N, int32_t F_total, int32_t max_faces, int32_t max_verts,
                                        const float *points, int32_t P, const int32_t *lengths, int32_t by_face, const int32_t *idx,
                                        const float *g, float *d_points, float *d_verts, void *workspace, void *stream_) {
    PmArgs a;
    const int rc = pm_fill(a, "smil_point_mesh_backward", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(vert_off && idx && g && d_points && d_verts, "smil_point_mesh_backward: null argument");
    SMIL_REQUIRE(max_verts >= 1 && max_verts <= n_verts, "smil_point_mesh_backward: max_verts=%d outside 1 .. V=%d", max_verts, n_verts);
    hipStream_t stream = (hipStream_t)stream_;
    a.vert_off = (const int *)vert_off; a.idx = (int *)idx; a.g = g; a.d_points = d_points; a.d_verts = d_verts; a.by_face = by_face != 0;
    const int rows = a.by_face ? max_faces : P;
    SMIL_HIP(hipMemsetAsync(a.dmax, 0, (size_t)N * sizeof(unsigned int), stream));
    SMIL_HIP(hipMemsetAsync(a.acc_v, 0, (size_t)n_verts * 3 * sizeof(long long), stream));
    if (a.by_face) SMIL_HIP(hipMemsetAsync(a.acc_p, 0, (size_t)N * P * 3 * sizeof(long long), stream));
    hipLaunchKernelGGL(k_pm_bwd_max, dim3(ceil_div(rows, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pm_bwd_add, dim3(ceil_div(rows, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pm_bwd_out, dim3(ceil_div(std::max(max_verts, a.by_face ? P : 1), 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
