// What the point <-> mesh kernels of point_mesh.hip share with the hierarchy of mesh_bvh.hip: the argument block, the mesh's ranges
// and power-of-two frame, the usability rules of faces and points, the workspace layout and the argument checks.  The kernels that
// write the frame's extent and face table and the float64 finish stay in point_mesh.hip; mesh_bvh.hip reaches them through
// pm_prepare() and pm_finish() below, so both searches run the same code on either side of "which face".
#pragma once

#include <algorithm>

#include "scan.h"
#include "point_tri.h"

struct PmArgs {
    const float *verts;       // (n_verts, 3) packed
    const int *faces;         // (F_total, 3) into the packed verts
    const int *face_off;      // (N + 1)
    const int *vert_off;      // (N + 1), the backward only
    const float *points;      // (N, P, 3)
    const int *lengths;       // (N) or NULL: P
    float4 *table;            // (F_total, 3) {v0, e1, e2} in the mesh's frame
    unsigned int *ext;        // (N) bits of the largest finite |coordinate| of mesh n
    unsigned long long *key;  // (N, P) or (F_total): scan.h's key of {d^2 in the frame, index}, minimum flavour
    float *dist2;             // (N, P) or (F_total)
    int *idx;                 // (N, P) face within its mesh or (F_total) point within its cloud, -1: none
    float *bary;              // (N, P, 3) or (F_total, 3)
    const float *g;           // upstream gradient per record
    long long *acc_v;         // (n_verts, 3)
    long long *acc_p;         // (N, P, 3); the winding numbers' integer sums are its first (N, P)
    float *winding;           // (N, P)
    unsigned int *dmax;       // (N) bits of the largest |2 g e| component of mesh n's records
    float *d_points;          // (N, P, 3)
    float *d_verts;           // (n_verts, 3)
    int N, P, n_verts, F_total, splits, by_face;
};

struct PmMesh { int f0, F, len; };  // first packed face, faces, points of mesh n

__device__ __forceinline__ PmMesh pm_mesh(const PmArgs &a, int n) {
    PmMesh m;
    m.f0 = min(max(a.face_off[n], 0), a.F_total);
    m.F = min(max(a.face_off[n + 1], m.f0), a.F_total) - m.f0;
    m.len = a.lengths ? min(max(a.lengths[n], 0), a.P) : a.P;
    return m;
}

__device__ __forceinline__ float pm_finite_abs(float x) { return fabsf(x) <= 3.0e38f ? fabsf(x) : 0.f; }  // NaN, inf: 0

// the three vertex ids of packed face j, or false when one is outside [0, n_verts)
__device__ __forceinline__ bool pm_face_ids(const PmArgs &a, size_t j, int (&id)[3]) {
    id[0] = a.faces[3 * j]; id[1] = a.faces[3 * j + 1]; id[2] = a.faces[3 * j + 2];
    return (unsigned)id[0] < (unsigned)a.n_verts && (unsigned)id[1] < (unsigned)a.n_verts && (unsigned)id[2] < (unsigned)a.n_verts;
}

// three coordinates are usable: none is NaN, inf or above 3e38, whatever a frame does to it
__device__ __forceinline__ bool pm_usable3(const float *p) { return fabsf(p[0]) <= 3.0e38f && fabsf(p[1]) <= 3.0e38f && fabsf(p[2]) <= 3.0e38f; }

// the nine coordinates of packed face j in the caller's units, or false when the face is not usable (an id out of range, a
// coordinate that is not usable)
__device__ __forceinline__ bool pm_face_coords(const PmArgs &a, size_t j, float (&c)[9]) {
    int id[3];
    if (!pm_face_ids(a, j, id)) return false;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        c[k] = a.verts[3 * (size_t)id[k / 3] + k % 3];
        finite &= fabsf(c[k]) <= 3.0e38f;
    }
    return finite;
}

// the frame of mesh n: coordinates are multiplied by 2^pm_frame (exactly)
__device__ __forceinline__ int pm_frame(const PmArgs &a, int n) { return -fix_max_exp(a.ext[n]); }

// A point in the frame; NaN (it never wins and nothing wins for it) when it is not usable, as for the vertices of a face.
__device__ __forceinline__ void pm_load_point(const float *p, int sh, float &x, float &y, float &z) {
    const bool usable = pm_usable3(p);
    const float nan = __builtin_nanf("");
    x = usable ? ldexpf(p[0], sh) : nan; y = usable ? ldexpf(p[1], sh) : nan; z = usable ? ldexpf(p[2], sh) : nan;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static size_t pm_layout(int N, int F_total, int P, int n_verts, char *base, PmArgs &a) {
    Workspace w{base};
    a.table = w.take<float4>((size_t)F_total * 3);
    a.key = w.take<unsigned long long>(std::max((size_t)N * P, (size_t)F_total));
    a.ext = w.take<unsigned int>((size_t)N);
    a.dmax = w.take<unsigned int>((size_t)N);
    a.acc_v = w.take<long long>((size_t)n_verts * 3);
    a.acc_p = w.take<long long>((size_t)N * P * 3);
    return w.used;
}

static bool pm_sizes_ok(int64_t N, int64_t F_total, int64_t P, int64_t n_verts) {
    return N > 0 && N <= 65535 && F_total > 0 && P > 0 && n_verts > 0 && N * P <= 0x7FFFFFFF / 4 && F_total <= 0x7FFFFFFF / 4 &&
           n_verts <= 0x7FFFFFFF / 4;
}

static int pm_fill(PmArgs &a, const char *who, const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                   int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths, void *workspace) {
    SMIL_REQUIRE(verts && faces && face_off && points && workspace, "%s: null argument", who);
    SMIL_REQUIRE(pm_sizes_ok(N, F_total, P, n_verts), "%s: bad sizes N=%d F=%d P=%d V=%d", who, N, F_total, P, n_verts);
    SMIL_REQUIRE(max_faces >= 1 && max_faces <= F_total, "%s: max_faces=%d outside 1 .. F=%d", who, max_faces, F_total);
    a = PmArgs{};
    pm_layout(N, F_total, P, n_verts, (char *)workspace, a);
    a.verts = verts; a.faces = (const int *)faces; a.face_off = (const int *)face_off; a.points = points; a.lengths = (const int *)lengths;
    a.N = N; a.P = P; a.n_verts = n_verts; a.F_total = F_total;
    return SMIL_OK;
}

// point_mesh.hip: what every forward search stands between.  pm_prepare clears the `n_keys` keys (0: the caller uses none) and
// writes the frame's extent (k_pm_extent) and the face table in the frame (k_pm_table); pm_finish writes the outputs of `rows`
// queries per mesh from the keys (k_pm_finish, float64).
int pm_prepare(PmArgs &a, int max_faces, size_t n_keys, hipStream_t stream);
int pm_finish(PmArgs &a, int rows, hipStream_t stream);
