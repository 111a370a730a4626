// A bounding-volume hierarchy over the faces of packed meshes, for gfx950: the nearest face of every point without the scan over all
// faces, and the SAME winner as point_mesh.hip's brute force, bit for bit.
//
// The tree of mesh n is implicit.  Its F faces stand in Morton order of their centroids (`order`: sorted position -> face within
// the mesh); SMIL_BVH_LEAF consecutive sorted faces make a leaf, L = ceil(F / SMIL_BVH_LEAF) leaves are padded to Lp, the next power
// of two (>= 1), and the 2 Lp - 1 nodes are numbered as a heap: the root is 1, the children of i are 2 i and 2 i + 1, leaf k is
// Lp + k.  Node i of mesh n is row bvh_node0(n) + i of `boxes` (row 0 of a mesh is not used).  No pointers and no atomics in the
// tree: two builds give the same bits.  A box is the exact float32 minimum and maximum of the vertices of the usable faces below
// it, in the caller's coordinates; without one it is EMPTY (+inf .. -inf) and is never entered.
//
//  * k_bvh_bounds   the bounding box of every mesh's usable faces (order-preserving integer atomicMin of float bits: the
//                   result does not depend on the order).
//  * k_bvh_codes    thread per face: the 30-bit Morton code of the centroid inside that box, as the int64 key {mesh, code}; a face
//                   that is not usable (point_mesh.h) gets the code SMIL_BVH_SENTINEL, behind every real one.  The host sorts the
//                   keys with a STABLE sort (ties keep face order) - plumbing - and hands back the permutation.
//  * k_bvh_order    the permutation as faces within their mesh; an entry that does not name a face of its mesh becomes -1.
//  * k_bvh_leaves   thread per leaf: the box of its faces.   k_bvh_level: thread per node of one level, bottom-up: the union of its
//                   two children.  refit = these two on new vertices in the stored order.  The answers never depend on the order's
//                   quality, only the number of visits does.
//  * k_bvh_gather   the face table of k_pm_table (point_mesh.hip, in this call's frame) copied into sorted order, so that a leaf's
//                   faces are consecutive 48-byte rows.
//  * k_bvh_points   lane = one point.  Depth first, nearer child first, WITHOUT a stack: in a heap the node still owed at level l is
//                   the sibling of the path's node at level l, so one bit per level (`owed`) is the whole traversal state - nothing
//                   is indexed dynamically and nothing can spill.  At a leaf: closest_on_triangle<float> on the rows of the table,
//                   the arithmetic of k_pm_points.  The running best is the key of scan.h, {d^2, face} compared lexicographically - what
//                   a sequential scan with a strict < selects - and a node is entered when its box's squared distance D^2 satisfies
//                   D^2 <= (sqrt(best) + EPS)^2 (1 + 2^-19): <=, never <, so that a float32 tie still reaches the smaller face
//                   index, and with the margin EPS for the float32 evaluation error of the leaf formula (bvh_visit_limit).
//  * then k_pm_finish (point_mesh.hip) in float64 on the same keys.
#include "point_mesh.h"

#define BVH_BLOCK 64
#define BVH_LEAF SMIL_BVH_LEAF

struct BvhArgs {
    PmArgs pm;
    const long long *perm;   // (F_total) sorted position -> packed face, from the host's sort
    long long *keys;         // (F_total) {mesh, Morton code}
    int *order;              // (F_total) sorted position -> face within its mesh
    float *boxes;            // (smil_bvh_nodes, 6) lo xyz, hi xyz
    float4 *sorted;          // (F_total, 3) pm.table in sorted order
    unsigned int *bounds;    // (N, 6) ordered bits of the meshes' boxes: lo xyz and -hi xyz, both minima
    long long *pkeys;        // (N, P) Morton codes of the points
    int *evaluated;          // (N, P) or NULL
    int level;               // k_bvh_level: the level written, counted from the leaves (1 = the leaves' parents)
};

struct BvhTree { int L, Lp, D; size_t node0; };  // leaves, padded leaves = 2^D, first row of `boxes`

__host__ __device__ static inline size_t bvh_node0(int f0, int n) { return 4 * ((size_t)(f0 / BVH_LEAF) + (size_t)n); }

__device__ __forceinline__ BvhTree bvh_tree(const PmMesh &m, int n) {
    BvhTree t;
    t.L = (m.F + BVH_LEAF - 1) / BVH_LEAF;
    t.D = t.L > 1 ? 32 - __clz(t.L - 1) : 0;
    t.Lp = 1 << t.D;
    t.node0 = bvh_node0(m.f0, n);  // (4 (floor(f1 / LEAF) - floor(f0 / LEAF) + 1) >= 4 L >= 2 Lp rows to the next mesh)
    return t;
}

// floats as unsigned integers of the same order (-inf lowest)
__device__ __forceinline__ unsigned int bvh_ordered(float x) {
    const unsigned int b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float bvh_unordered(unsigned int o) { return __uint_as_float((o & 0x80000000u) ? o & 0x7FFFFFFFu : ~o); }

// the vertices of face `t` of mesh m when there is such a face and it is usable (point_mesh.h)
__device__ __forceinline__ bool bvh_face(const PmArgs &a, const PmMesh &m, int t, float (&c)[9]) {
    return t >= 0 && t < m.F && pm_face_coords(a, (size_t)m.f0 + t, c);
}

struct BvhBox { float lo[3], hi[3]; };

__device__ __forceinline__ BvhBox bvh_empty() {
    BvhBox b;
#pragma unroll
    for (int k = 0; k < 3; ++k) { b.lo[k] = __builtin_inff(); b.hi[k] = -__builtin_inff(); }
    return b;
}
__device__ __forceinline__ void bvh_grow(BvhBox &b, const float (&c)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { b.lo[k % 3] = fminf(b.lo[k % 3], c[k]); b.hi[k % 3] = fmaxf(b.hi[k % 3], c[k]); }
}

// (every lane of every wave reaches the folds)
__global__ void __launch_bounds__(256) k_bvh_bounds(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    BvhBox box = bvh_empty();
    float c[9];
    if (bvh_face(a, m, t, c)) bvh_grow(box, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = wave_fold(box.lo[k], [](float x, float y) { return fminf(x, y); });
        const float hi = wave_fold(box.hi[k], [](float x, float y) { return fmaxf(x, y); });
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&b.bounds[6 * n + k], bvh_ordered(lo));
            atomicMin(&b.bounds[6 * n + 3 + k], bvh_ordered(-hi));
        }
    }
}

__device__ __forceinline__ unsigned int bvh_spread10(unsigned int x) {  // bit i of 10 -> bit 3 i
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// the Morton code of (x, y, z) inside lo .. hi, 10 bits an axis (halved first: hi - lo cannot overflow; an axis of extent 0: cell 0)
__device__ __forceinline__ unsigned int bvh_morton(const float (&p)[3], const float (&lo)[3], const float (&hi)[3]) {
    unsigned int code = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = (0.5f * p[k] - 0.5f * lo[k]) / (0.5f * hi[k] - 0.5f * lo[k]);
        const int q = (int)(pt_clamp(t, 0.f, 1.f) * 1023.f);  // (NaN clamps to 0)
        code |= bvh_spread10((unsigned int)q) << k;
    }
    return code;
}

__global__ void __launch_bounds__(256) k_bvh_codes(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    if (t >= m.F) return;
    float c[9], lo[3], hi[3];
    unsigned int code = SMIL_BVH_SENTINEL;
    if (bvh_face(a, m, t, c)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = bvh_unordered(b.bounds[6 * n + k]); hi[k] = -bvh_unordered(b.bounds[6 * n + 3 + k]); }
        const float third = 1.f / 3.f;
        const float mid[3] = {c[0] * third + c[3] * third + c[6] * third, c[1] * third + c[4] * third + c[7] * third,
                              c[2] * third + c[5] * third + c[8] * third};
        code = bvh_morton(mid, lo, hi);
    }
    b.keys[(size_t)m.f0 + t] = ((long long)n << 32) | (long long)code;
}

__global__ void __launch_bounds__(256) k_bvh_order(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    if (t >= m.F) return;
    const long long j = b.perm[(size_t)m.f0 + t] - m.f0;
    b.order[(size_t)m.f0 + t] = j >= 0 && j < m.F ? (int)j : -1;
}

__device__ __forceinline__ void bvh_store(float *row, const BvhBox &box) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { row[k] = box.lo[k]; row[3 + k] = box.hi[k]; }
}

// thread per padded leaf: a leaf beyond L, and one whose faces are all unusable, is empty
__global__ void __launch_bounds__(256) k_bvh_leaves(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    const BvhTree tr = bvh_tree(m, n);
    if (t >= tr.Lp) return;
    BvhBox box = bvh_empty();
    float c[9];
    for (int s = t * BVH_LEAF; s < min(m.F, (t + 1) * BVH_LEAF); ++s)  // (t < Lp <= 2 L: t * LEAF does not overflow)
        if (bvh_face(a, m, b.order[(size_t)m.f0 + s], c)) bvh_grow(box, c);
    bvh_store(b.boxes + 6 * (tr.node0 + tr.Lp + t), box);
}

// thread per node of the level `b.level` above the leaves: nodes [Lp >> level, 2 (Lp >> level))
__global__ void __launch_bounds__(256) k_bvh_level(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const BvhTree tr = bvh_tree(pm_mesh(a, n), n);
    if (b.level > tr.D) return;
    const int first = tr.Lp >> b.level;
    if (t >= first) return;
    const size_t i = (size_t)first + t;
    const float *l = b.boxes + 6 * (tr.node0 + 2 * i), *r = l + 6;
    BvhBox box;
#pragma unroll
    for (int k = 0; k < 3; ++k) { box.lo[k] = fminf(l[k], r[k]); box.hi[k] = fmaxf(l[3 + k], r[3 + k]); }
    bvh_store(b.boxes + 6 * (tr.node0 + i), box);
}

__global__ void __launch_bounds__(256) k_bvh_gather(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMesh m = pm_mesh(a, n);
    if (t >= m.F) return;
    const size_t at = (size_t)m.f0 + t;
    const int j = b.order[at];
    const float nan = __builtin_nanf("");
    const bool ok = j >= 0 && j < m.F;  // (a row that names no face never wins, as an unusable face)
    const float4 *row = a.table + 3 * ((size_t)m.f0 + (ok ? j : 0));
    b.sorted[3 * at] = ok ? row[0] : make_float4(nan, nan, nan, 0.f);
    b.sorted[3 * at + 1] = row[1];
    b.sorted[3 * at + 2] = row[2];
}

// The squared distance of the frame's point to a box given in the caller's coordinates (scaled by the frame's power of two, which
// is exact and monotone); +inf for an empty box.
__device__ __forceinline__ float bvh_box_d2(const float *row, int sh, float px, float py, float pz) {
    const float dx = fmaxf(fmaxf(ldexpf(row[0], sh) - px, px - ldexpf(row[3], sh)), 0.f);
    const float dy = fmaxf(fmaxf(ldexpf(row[1], sh) - py, py - ldexpf(row[4], sh)), 0.f);
    const float dz = fmaxf(fmaxf(ldexpf(row[2], sh) - pz, pz - ldexpf(row[5], sh)), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

// The largest computed box distance D^2 at which a node may still hold a face whose float32 d^2 is <= best.
// Every face below the node lies in its box, so its true distance d* >= D.  The leaf formula's float32 value cannot be below d*^2 by
// more than its evaluation error, 6.5 u L on d (section 4.20; the computed point is ON the face), and in the frame every coordinate is
// below 1, so L <= 2 sqrt 3 and the error is below 22.6 u = 2^-19.5; EPS = 2^-18 doubles that twice over for the terms beyond first
// order.  So sqrt(d^2 computed) <= sqrt(best) needs D <= sqrt(best) + EPS.  The computed D^2 exceeds the true one by at most 6 u
// relative (three rounded differences squared and summed) and the limit below falls short of the true one by at most 4 u: the factor
// 1 + 2^-19 = 1 + 32 u covers both.  best = +inf gives +inf: everything is entered until a face has been evaluated.
#define BVH_EPS 3.814697265625e-06f  // 2^-18
__device__ __forceinline__ float bvh_visit_limit(float best) {
    const float s = sqrtf(best) + BVH_EPS;
    return s * s * 1.0000019073486328125f;  // 1 + 2^-19
}

__global__ void __launch_bounds__(BVH_BLOCK) k_bvh_points(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y;
    const PmMesh m = pm_mesh(a, n);
    const int q = blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (q >= m.len || m.F == 0) return;  // (a padded point and a mesh without faces keep the cleared key: +inf, -1, 0)
    const BvhTree tr = bvh_tree(m, n);
    const int sh = pm_frame(a, n);
    float px, py, pz;
    pm_load_point(a.points + ((size_t)n * a.P + q) * 3, sh, px, py, pz);
    float best = __builtin_inff(), limit = __builtin_inff();
    int bi = 0x7FFFFFFF, count = 0;
    if (px == px) {  // (an unusable point is NaN in the frame: nothing wins for it, and no box distance means anything)
        const float *boxes = b.boxes + 6 * tr.node0;
        const float4 *table = b.sorted + 3 * (size_t)m.f0;
        const int *order = b.order + m.f0;
        unsigned int i = 1, owed = 0;  // the node, and bit l: the sibling of the path's node at level l is still to be entered
        bool down = true;
        while (true) {
            if (down) {
                const int level = 31 - __clz(i);
                if (level == tr.D) {  // a leaf
                    const int s0 = (int)(i - tr.Lp) * BVH_LEAF, s1 = min(m.F, s0 + BVH_LEAF);
                    for (int s = s0; s < s1; ++s) {
                        const float4 v0 = table[3 * (size_t)s], e1 = table[3 * (size_t)s + 1], e2 = table[3 * (size_t)s + 2];
                        const TriPoint<float> r = closest_on_triangle<float>(px - v0.x, py - v0.y, pz - v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
                        const int f = order[s];
                        const bool take = r.dist2 < best || (r.dist2 == best && f < bi);
                        best = take ? r.dist2 : best;
                        bi = take ? f : bi;
                    }
                    count += max(s1 - s0, 0);
                    limit = bvh_visit_limit(best);
                    down = false;
                } else {
                    const float d0 = bvh_box_d2(boxes + 6 * (size_t)(2 * i), sh, px, py, pz);
                    const float d1 = bvh_box_d2(boxes + 6 * (size_t)(2 * i + 1), sh, px, py, pz);
                    const bool in0 = d0 <= limit && d0 < __builtin_inff(), in1 = d1 <= limit && d1 < __builtin_inff();
                    if (in0 || in1) {
                        const bool right = in1 && (!in0 || d1 < d0);
                        if (in0 && in1) owed |= 1u << (level + 1);
                        i = 2 * i + (right ? 1u : 0u);
                    } else {
                        down = false;
                    }
                }
            } else {
                if (owed == 0) break;
                const int l = 31 - __clz(owed);  // the deepest level that owes: never below the node's own
                owed &= ~(1u << l);
                i = (i >> ((31 - __clz(i)) - l)) ^ 1u;
                const float d = bvh_box_d2(boxes + 6 * (size_t)i, sh, px, py, pz);  // once more: best has fallen since
                down = d <= limit && d < __builtin_inff();
            }
        }
    }
    if (b.evaluated) b.evaluated[(size_t)n * a.P + q] = count;
    if (best < __builtin_inff()) scan_put_min(&a.key[(size_t)n * a.P + q], 1, best, bi);  // (one traversal per point: no splits)
}

// the Morton code of every point inside its mesh's root box, for callers that present the queries in spatial order; a point that is
// padded or not usable gets the sentinel
__global__ void __launch_bounds__(256) k_bvh_point_codes(BvhArgs b) {
    const PmArgs &a = b.pm;
    const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.P) return;
    const PmMesh m = pm_mesh(a, n);
    const float *root = b.boxes + 6 * (bvh_tree(m, n).node0 + 1);
    const float *p = a.points + ((size_t)n * a.P + t) * 3;
    const bool usable = t < m.len && pm_usable3(p);
    const float x[3] = {p[0], p[1], p[2]}, lo[3] = {root[0], root[1], root[2]}, hi[3] = {root[3], root[4], root[5]};
    b.pkeys[(size_t)n * a.P + t] = usable ? (long long)bvh_morton(x, lo, hi) : (long long)SMIL_BVH_SENTINEL;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static size_t bvh_layout(int N, int F_total, int P, int n_verts, char *base, BvhArgs &b) {
    Workspace w{base};
    w.used = pm_layout(N, F_total, P, n_verts, base, b.pm);
    b.sorted = w.take<float4>((size_t)F_total * 3);
    b.bounds = w.take<unsigned int>((size_t)N * 6);
    return w.used;
}

extern "C" size_t smil_bvh_workspace_bytes(int32_t N, int32_t F_total, int32_t P, int32_t n_verts) {
    BvhArgs b;
    return pm_sizes_ok(N, F_total, P, n_verts) ? bvh_layout(N, F_total, P, n_verts, nullptr, b) : 0;
}

extern "C" size_t smil_bvh_nodes(int32_t N, int32_t F_total) {
    return pm_sizes_ok(N, F_total, 1, 1) ? bvh_node0(F_total, N) : 0;
}

// `points` may be NULL (build, refit): the cloud is then the one point the workspace was sized for and is never read
static int bvh_fill(BvhArgs &b, const char *who, const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                    int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths, void *workspace) {
    b = BvhArgs{};
    const int rc = pm_fill(b.pm, who, verts, n_verts, faces, face_off, N, F_total, max_faces, points ? points : verts, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    bvh_layout(N, F_total, P, n_verts, (char *)workspace, b);
    return SMIL_OK;
}

// the leaf boxes, then the levels above them, bottom-up, for the deepest tree any mesh can have
static int bvh_boxes(BvhArgs &b, int max_faces, hipStream_t stream) {
    const int L = ceil_div(max_faces, BVH_LEAF);
    int D = 0;
    while ((1 << D) < L) ++D;
    hipLaunchKernelGGL(k_bvh_leaves, dim3(ceil_div(1 << D, 256), b.pm.N), dim3(256), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    for (b.level = 1; b.level <= D; ++b.level) {
        hipLaunchKernelGGL(k_bvh_level, dim3(ceil_div((1 << D) >> b.level, 256), b.pm.N), dim3(256), 0, stream, b);
        SMIL_LAUNCH_CHECK();
    }
    return SMIL_OK;
}

extern "C" int smil_bvh_codes(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                              int32_t max_faces, int64_t *keys, void *workspace, void *stream_) {
    BvhArgs b;
    const int rc = bvh_fill(b, "smil_bvh_codes", verts, n_verts, faces, face_off, N, F_total, max_faces, nullptr, 1, nullptr, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(keys, "smil_bvh_codes: null output");
    hipStream_t stream = (hipStream_t)stream_;
    b.keys = (long long *)keys;
    SMIL_HIP(hipMemsetAsync(b.bounds, 0xFF, (size_t)N * 6 * sizeof(unsigned int), stream));  // above every float's ordered bits
    hipLaunchKernelGGL(k_bvh_bounds, dim3(ceil_div(max_faces, 256), N), dim3(256), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bvh_codes, dim3(ceil_div(max_faces, 256), N), dim3(256), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_bvh_build(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                              int32_t max_faces, const int64_t *perm, int32_t *order, float *boxes, void *workspace, void *stream_) {
    BvhArgs b;
    const int rc = bvh_fill(b, "smil_bvh_build", verts, n_verts, faces, face_off, N, F_total, max_faces, nullptr, 1, nullptr, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(perm && order && boxes, "smil_bvh_build: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    b.perm = (const long long *)perm; b.order = (int *)order; b.boxes = boxes;
    hipLaunchKernelGGL(k_bvh_order, dim3(ceil_div(max_faces, 256), N), dim3(256), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    return bvh_boxes(b, max_faces, stream);
}

extern "C" int smil_bvh_refit(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                              int32_t max_faces, const int32_t *order, float *boxes, void *workspace, void *stream_) {
    BvhArgs b;
    const int rc = bvh_fill(b, "smil_bvh_refit", verts, n_verts, faces, face_off, N, F_total, max_faces, nullptr, 1, nullptr, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(order && boxes, "smil_bvh_refit: null argument");
    b.order = (int *)order; b.boxes = boxes;
    return bvh_boxes(b, max_faces, (hipStream_t)stream_);
}

extern "C" int smil_bvh_point_codes(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                    int32_t F_total, int32_t max_faces, const float *boxes, const float *points, int32_t P,
                                    const int32_t *lengths, int64_t *keys, void *workspace, void *stream_) {
    BvhArgs b;
    const int rc = bvh_fill(b, "smil_bvh_point_codes", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths, workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(boxes && points && keys, "smil_bvh_point_codes: null argument");
    b.boxes = (float *)boxes; b.pkeys = (long long *)keys;
    hipLaunchKernelGGL(k_bvh_point_codes, dim3(ceil_div(P, 256), N), dim3(256), 0, (hipStream_t)stream_, b);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_bvh_point_face_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                            int32_t F_total, int32_t max_faces, const int32_t *order, const float *boxes,
                                            const float *points, int32_t P, const int32_t *lengths, float *dist2, int32_t *face,
                                            float *bary, int32_t *evaluated, void *workspace, void *stream_) {
    BvhArgs b;
    const int rc = bvh_fill(b, "smil_bvh_point_face_distance", verts, n_verts, faces, face_off, N, F_total, max_faces, points, P, lengths,
                            workspace);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(order && boxes && points && dist2 && face && bary, "smil_bvh_point_face_distance: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    PmArgs &a = b.pm;
    a.dist2 = dist2; a.idx = (int *)face; a.bary = bary; a.by_face = 0; a.splits = 1;
    b.order = (int *)order; b.boxes = (float *)boxes; b.evaluated = (int *)evaluated;
    int rc2 = pm_prepare(a, max_faces, (size_t)N * P, stream);
    if (rc2 != SMIL_OK) return rc2;
    if (evaluated) SMIL_HIP(hipMemsetAsync(evaluated, 0, (size_t)N * P * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_bvh_gather, dim3(ceil_div(max_faces, 256), N), dim3(256), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bvh_points, dim3(ceil_div(P, BVH_BLOCK), N), dim3(BVH_BLOCK), 0, stream, b);
    SMIL_LAUNCH_CHECK();
    return pm_finish(a, P, stream);
}
