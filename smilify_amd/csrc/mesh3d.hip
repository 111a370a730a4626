// 3-D scan registration losses for gfx950: the loss half of the reference's fitter_3d/trainer.py Stage.forward (:368-388).
//
// Replaces (reference): pytorch3d 0.7.8 (un-vendored) ops.sample_points_from_meshes, loss.chamfer_distance, loss.mesh_edge_loss,
// loss.mesh_normal_consistency and loss.mesh_laplacian_smoothing(method="uniform"), as fitter_3d/trainer.py:3-9 imports them.
//
//  * k_sample_points     lane per sample: a counter-based Philox4x32-10 draw keyed by (seed, mesh, sample), the face by binary search
//                        in the mesh's normalised cumulative-area table (float64, built once on the host), barycentrics
//                        w0 = 1 - sqrt(u), w1 = sqrt(u)(1 - v), w2 = sqrt(u) v (pytorch3d _rand_barycentric_coords).
//  * k_chamfer_nn        lane = CH_QPT query points, both directions in one launch; candidates stream through LDS as float4 and every
//                        lane reads the same one (a broadcast).  Direct form sum (q - c)^2, running min with a strict <.  Candidate
//                        ranges may be split across workgroups; the splits merge in the query's key, minimum flavour.  The key, the
//                        split's range and count and the staging are scan.h's, as for k_knn, raycast.hip and point_mesh.hip.
//  * k_chamfer_owned     thread per query: argmin out, the owned gradient 2 w (q - c*), and the scattered side (c* - q) added to the
//                        candidate's int64 fixed-point accumulator, whose unit follows the largest minimum found and the number
//                        of queries of its (mesh, direction): ch_fix_exp, and "order-independent scatter sums" in common.h.
//  * k_chamfer_scatter   thread per point: the scattered sum converted and added to the owned gradient.
//  * k_chamfer_reduce    per (mesh, direction) sums of the minima in a fixed order, then the batch in a fixed order.
//  * k_mesh_reg          edge, normal consistency and uniform Laplacian terms and their gradients in one pass: thread t evaluates edge
//                        term t, normal pair t and Laplacian row t for the loss, and gathers vertex t's gradient from its neighbour and
//                        pair incidence lists (recomputing the few terms it touches: no atomics).  Per-block partials, then
//                        k_mesh_reg_reduce in a fixed order.
//
// The SDF-guided term (reference fitter_3d/utils.py:973-1394, trainer.py:398-433), see the section at the end of the file:
//  * k_knn               wave = KNN_QPW queries, both directions in one launch.  A query's K-list is spread over the wave's lanes as
//                        keys (scan.h), ascending; lane l takes candidate c0 + l of every 64 of a tile (scan_tiles), and a
//                        candidate enters a list only when its key is below the list's K-th (one compare and a ballot per query).
//  * k_sdf_stats         per (mesh, side) mean and unbiased std of the values in two float64 passes, then the z-scores.
//  * k_sdf_term          wave per query, lane per neighbour: softmax weights, r_i, the owned gradient, and the scattered gradient into
//                        the chamfer path's int64 fixed-point accumulators (k_chamfer_scatter / _reduce / _total finish the call).
//  * k_sample_vertices   lane per sample: a Philox draw keyed by (seed, mesh, sample), index = (r * V_n) >> 32, points and values
//                        gathered; k_sv_* scatter a gradient on the samples back to the vertices as int64 fixed point.
#include <algorithm>

#include "scan.h"

#define CH_BLOCK 256
#define CH_QPT 4                      // query points per lane of k_chamfer_nn
#define CH_TILE 256                   // candidates staged in LDS per step
#define REG_BLOCK 256

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// ---------------------------------------------------------------------------------------------
// surface sampling
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sample_points(const float *__restrict__ verts, const int *__restrict__ faces,
                                                       const int *__restrict__ face_off, const double *__restrict__ cum, int S,
                                                       uint32_t seed_lo, uint32_t seed_hi, float *__restrict__ out,
                                                       int *__restrict__ out_face) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = blockIdx.y;
    if (s >= S) return;
    const size_t o = (size_t)n * S + s;
    const int f0 = face_off[n], f1 = face_off[n + 1];
    if (f1 <= f0 || !(cum[f1 - 1] > 0.0)) {  // no faces / no area: zeros (pytorch3d leaves empty meshes' samples at 0)
        out[3 * o] = 0.f; out[3 * o + 1] = 0.f; out[3 * o + 2] = 0.f;
        if (out_face) out_face[o] = -1;
        return;
    }
    const uint4 r = philox4x32_10(make_uint4((uint32_t)s, (uint32_t)n, 0u, 0u), make_uint2(seed_lo, seed_hi));
    const double uf = (double)(((uint64_t)r.x << 21) ^ (uint64_t)(r.y >> 11)) * (1.0 / 9007199254740992.0);  // [0, 1), 53 bits
    // first face whose cumulative (normalised) area exceeds uf: zero-area faces are never chosen
    int lo = f0, hi = f1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > uf) hi = mid;
        else lo = mid + 1;
    }
    const float u = (float)(r.z >> 8) * (1.0f / 16777216.0f), v = (float)(r.w >> 8) * (1.0f / 16777216.0f);
    const float su = sqrtf(u);
    const float w0 = 1.0f - su, w1 = su * (1.0f - v), w2 = su * v;
    const float *a = verts + 3 * (size_t)faces[3 * lo], *b = verts + 3 * (size_t)faces[3 * lo + 1], *c = verts + 3 * (size_t)faces[3 * lo + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * o + k] = w0 * a[k] + w1 * b[k] + w2 * c[k];
    if (out_face) out_face[o] = lo - f0;
}

extern "C" int smil_sample_points(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, const double *cum_area,
                                  int32_t N, int32_t S, uint64_t seed, float *out, int32_t *out_face, void *stream_) {
    SMIL_REQUIRE(verts && faces && face_off && cum_area && out, "smil_sample_points: null argument");
    SMIL_REQUIRE(N > 0 && S > 0 && n_verts > 0, "smil_sample_points: bad sizes N=%d S=%d V=%d", N, S, n_verts);
    SMIL_REQUIRE(N <= 65535, "smil_sample_points: N=%d meshes exceeds one launch (65535)", N);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_sample_points, dim3(ceil_div(S, 256), N), dim3(256), 0, stream, verts, (const int *)faces, (const int *)face_off,
                       cum_area, S, (uint32_t)seed, (uint32_t)(seed >> 32), out, (int *)out_face);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---------------------------------------------------------------------------------------------
// chamfer distance
// ---------------------------------------------------------------------------------------------
// What chamfer and the SDF term share: two clouds, a per-query distance, its loss, and the gradient of both clouds.  (Pointers
// before sizes: the other way round hipcc 7.2 gives k_chamfer_nn 76 VGPRs for 47.)
struct CloudLossArgs {
    const float *pts[2];      // (N, P[d], 3): direction d's queries are pts[d], its candidates pts[1 - d]
    float *dist;              // (N, P[0] + P[1]) direction 0's queries first: the minimum (chamfer), r_i (the SDF term)
    long long *acc;           // (N, P[0] + P[1], 3) fixed-point scattered sums, per point of either cloud
    unsigned int *dmax;       // (N, 2) bits of the largest squared distance of (mesh, direction) that enters a gradient
    float *grad[2];           // (N, P[d], 3) or NULL
    float *part;              // (N, dirs)
    float *loss;              // (1)
    int P[2];
    int N, dirs;
    int K;                    // terms of one query that can meet in a scattered sum's point: 1 (chamfer), K (the SDF term)
    float w[2];               // loss weight of one term of direction d (1/P and/or 1/N as reduced)
};

// ... and what only the nearest-neighbour search of chamfer uses
struct ChamferArgs : CloudLossArgs {
    int splits;
    unsigned long long *key;  // (N, P[0] + P[1]) {distance bits, candidate index}: direction 0's queries first
    int *idx[2];              // (N, P[d]) or NULL
};

__device__ __forceinline__ size_t ch_row(const CloudLossArgs &a, int n, int d) { return (size_t)n * (a.P[0] + a.P[1]) + (d ? a.P[0] : 0); }

// Unit exponent (common.h) of direction d's scattered sums in mesh n.  Magnitude: the half exponent of the largest squared distance plus
// one (for the rounding of the distance), which bounds every component of q - c*.  Addends: P[d] K (the SDF term's weigh <= 1).
__device__ __forceinline__ int ch_fix_exp(const CloudLossArgs &a, int n, int d) {
    return fix_unit_exp(((fix_max_exp(a.dmax[n * 2 + d]) + 1) >> 1) + 1, (long long)a.P[d] * a.K);
}

__global__ void __launch_bounds__(CH_BLOCK) k_chamfer_nn(ChamferArgs a) {
    __shared__ float4 tile[CH_TILE];
    const int d = blockIdx.z % a.dirs, n = blockIdx.z / a.dirs;
    const int Pq = a.P[d], Pc = a.P[1 - d];
    const int q0 = blockIdx.x * (CH_BLOCK * CH_QPT);
    if (q0 >= Pq) return;  // (block-uniform)
    int c_begin, c_end;
    scan_split_range(Pc, a.splits, CH_TILE, c_begin, c_end);
    if (c_begin >= c_end) return;
    const float *Q = a.pts[d] + (size_t)n * Pq * 3;
    const float *C = a.pts[1 - d] + (size_t)n * Pc * 3;
    float qx[CH_QPT], qy[CH_QPT], qz[CH_QPT], best[CH_QPT];
    int bi[CH_QPT];
#pragma unroll
    for (int k = 0; k < CH_QPT; ++k) {
        const int q = q0 + k * CH_BLOCK + threadIdx.x;
        const int qc = q < Pq ? q : Pq - 1;
        qx[k] = Q[3 * qc]; qy[k] = Q[3 * qc + 1]; qz[k] = Q[3 * qc + 2];
        best[k] = __builtin_inff();
        bi[k] = 0x7FFFFFFF;
    }
    for (int c0 = c_begin; c0 < c_end; c0 += CH_TILE) {  // (scan_tiles written out: as a lambda the body costs 19 VGPRs and a wave)
        const int cnt = min(CH_TILE, c_end - c0);
        scan_stage(tile, ScanStageXyz{C}, c0, cnt);
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 c = tile[j];
#pragma unroll
            for (int k = 0; k < CH_QPT; ++k) {
                const float dx = qx[k] - c.x, dy = qy[k] - c.y, dz = qz[k] - c.z;
                const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (dd < best[k]) { best[k] = dd; bi[k] = c0 + j; }
            }
        }
    }
    unsigned long long *key = a.key + ch_row(a, n, d);
    float bmax = 0.f;
#pragma unroll
    for (int k = 0; k < CH_QPT; ++k) {
        const int q = q0 + k * CH_BLOCK + threadIdx.x;
        if (q < Pq) {
            scan_put_min(&key[q], a.splits, best[k], bi[k]);
            bmax = fmaxf(bmax, best[k]);
        }
    }
    if (a.grad[0]) fix_record_max(&a.dmax[n * 2 + d], bmax);
}

__global__ void __launch_bounds__(256) k_chamfer_owned(ChamferArgs a) {
    const int d = blockIdx.z % a.dirs, n = blockIdx.z / a.dirs;
    const int Pq = a.P[d], Pc = a.P[1 - d];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Pq) return;
    const size_t r = ch_row(a, n, d) + q;
    const unsigned long long kv = a.key[r];
    const int j = scan_key_index(kv);
    a.dist[r] = scan_key_value(kv);
    if (a.idx[d]) a.idx[d][(size_t)n * Pq + q] = j;
    if (!a.grad[0]) return;
    if (j < 0 || j >= Pc) return;  // (every query sees at least one candidate: P >= 1 is checked on the host)
    const float *Q = a.pts[d] + ((size_t)n * Pq + q) * 3;
    const float *Cp = a.pts[1 - d] + ((size_t)n * Pc + j) * 3;
    const float e[3] = {Q[0] - Cp[0], Q[1] - Cp[1], Q[2] - Cp[2]};
    if (a.grad[d]) {
        float *g = a.grad[d] + ((size_t)n * Pq + q) * 3;
        const float s = 2.0f * a.w[d];
        g[0] = s * e[0]; g[1] = s * e[1]; g[2] = s * e[2];
    }
    if (a.grad[1 - d]) {  // candidate j receives 2 w_d (c - q): accumulated as integers, so the order of the additions does not matter
        long long *acc = a.acc + (ch_row(a, n, 1 - d) + j) * 3;
        const int fix = ch_fix_exp(a, n, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(&acc[k], -(double)e[k], fix);
    }
}

// both clouds' points: the scattered sums of direction 1 - s land on cloud s's points, weighted by w[1 - s]
__global__ void __launch_bounds__(256) k_chamfer_scatter(CloudLossArgs a) {
    const int side = blockIdx.z & 1, n = blockIdx.z >> 1;
    const int P = a.P[side];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P || !a.grad[side]) return;
    const bool has_owned = side < a.dirs;  // (single_directional: cloud 1 owns no term)
    const bool receives = 1 - side < a.dirs;
    float *g = a.grad[side] + ((size_t)n * P + i) * 3;
    const long long *acc = a.acc + (ch_row(a, n, side) + i) * 3;
    const float s = receives ? 2.0f * a.w[1 - side] : 0.f;
    const int fix = receives ? ch_fix_exp(a, n, 1 - side) : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sc = receives ? fix_read(acc[k], fix) * s : 0.f;
        g[k] = (has_owned ? g[k] : 0.f) + sc;
    }
}

__global__ void __launch_bounds__(256) k_chamfer_reduce(CloudLossArgs a) {
    __shared__ float red[16];
    const int d = blockIdx.x % a.dirs, n = blockIdx.x / a.dirs;
    const int P = a.P[d];
    const float *dist = a.dist + ch_row(a, n, d);
    float s = 0.f;
    for (int i = threadIdx.x; i < P; i += blockDim.x) s += dist[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.part[blockIdx.x] = s * a.w[d];
}

__global__ void __launch_bounds__(64) k_chamfer_total(const float *__restrict__ part, int n, float *__restrict__ loss) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = s;
}

// the shared part but its workspace regions and K
static void cloud_loss_fill(CloudLossArgs &c, const float *x, const float *y, int N, int P1, int P2, int single_directional, int point_sum,
                            int batch_sum, float *d_x, float *d_y, float *loss) {
    c.pts[0] = x; c.pts[1] = y;
    c.P[0] = P1; c.P[1] = P2;
    c.N = N; c.dirs = single_directional ? 1 : 2;
    const float bw = batch_sum ? 1.0f : 1.0f / (float)N;
    c.w[0] = (point_sum ? 1.0f : 1.0f / (float)P1) * bw;
    c.w[1] = (point_sum ? 1.0f : 1.0f / (float)P2) * bw;
    c.grad[0] = d_x; c.grad[1] = d_y;
    c.loss = loss;
}

// the end of both calls: the scattered sums into the gradients, then the loss from c.dist
static int cloud_loss_finish(const CloudLossArgs &c, hipStream_t stream) {
    if (c.grad[0]) {
        hipLaunchKernelGGL(k_chamfer_scatter, dim3(ceil_div(std::max(c.P[0], c.P[1]), 256), 1, c.N * 2), dim3(256), 0, stream, c);
        SMIL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_chamfer_reduce, dim3(c.N * c.dirs), dim3(256), 0, stream, c);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chamfer_total, dim3(1), dim3(64), 0, stream, (const float *)c.part, c.N * c.dirs, c.loss);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

static size_t chamfer_layout(int N, int P1, int P2, char *base, ChamferArgs &a) {
    const size_t pts = (size_t)N * ((size_t)P1 + P2);
    Workspace w{base};
    a.key = w.take<unsigned long long>(pts);
    a.dist = w.take<float>(pts);
    a.acc = w.take<long long>(pts * 3);
    a.part = w.take<float>((size_t)N * 2);
    a.dmax = w.take<unsigned int>((size_t)N * 2);
    return w.used;
}

extern "C" size_t smil_chamfer_workspace_bytes(int32_t N, int32_t P1, int32_t P2) {
    ChamferArgs a;
    return (N > 0 && P1 > 0 && P2 > 0) ? chamfer_layout(N, P1, P2, nullptr, a) : 0;
}

extern "C" int smil_chamfer(const float *x, const float *y, int32_t N, int32_t P1, int32_t P2, int32_t single_directional,
                            int32_t point_sum, int32_t batch_sum, float *loss, int32_t *idx_x, int32_t *idx_y, float *d_x, float *d_y,
                            void *workspace, void *stream_) {
    SMIL_REQUIRE(x && y && loss && workspace, "smil_chamfer: null argument");
    SMIL_REQUIRE(N > 0 && P1 > 0 && P2 > 0, "smil_chamfer: bad sizes N=%d P1=%d P2=%d", N, P1, P2);
    SMIL_REQUIRE(N <= 32767, "smil_chamfer: N=%d exceeds one launch (32767)", N);
    SMIL_REQUIRE((d_x == nullptr) == (d_y == nullptr), "smil_chamfer: d_x and d_y are given together or not at all");
    SMIL_REQUIRE(!(single_directional && idx_y), "smil_chamfer: idx_y has no meaning when single_directional");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t pts = (size_t)N * ((size_t)P1 + P2);
    ChamferArgs a;
    chamfer_layout(N, P1, P2, (char *)workspace, a);
    cloud_loss_fill(a, x, y, N, P1, P2, single_directional, point_sum, batch_sum, d_x, d_y, loss);
    a.K = 1;
    a.idx[0] = idx_x; a.idx[1] = idx_y;
    // candidate splits: >= 2048 workgroups while every split still streams >= 4 tiles
    const int qblocks = ceil_div(std::max(P1, P2), CH_BLOCK * CH_QPT);
    a.splits = scan_splits(0, qblocks * N * a.dirs, std::min(P1, P2), CH_TILE, 4, 2048);
    SMIL_HIP(hipMemsetAsync(a.key, 0xFF, pts * 8, stream));
    if (d_x) {
        SMIL_HIP(hipMemsetAsync(a.acc, 0, pts * 3 * 8, stream));
        SMIL_HIP(hipMemsetAsync(a.dmax, 0, (size_t)N * 2 * sizeof(unsigned int), stream));
    }
    hipLaunchKernelGGL(k_chamfer_nn, dim3(qblocks, a.splits, N * a.dirs), dim3(CH_BLOCK), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chamfer_owned, dim3(ceil_div(std::max(P1, P2), 256), 1, N * a.dirs), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return cloud_loss_finish(a, stream);
}

// ---------------------------------------------------------------------------------------------
// mesh regularisers (shared topology of B meshes)
// ---------------------------------------------------------------------------------------------
struct RegArgs {
    SmilMeshTopology t;
    const float *verts;  // (B, V, 3)
    int B, terms;
    float *d_edge, *d_normal, *d_lap;  // (B, V, 3) or NULL
    float *part;                       // (B, nblk, 3)
    float *out;                        // (3): edge, normal, laplacian
    float *per_mesh;                   // (B, 3)
};

__device__ __forceinline__ void ld3(const float *X, int v, float (&p)[3]) { p[0] = X[3 * v]; p[1] = X[3 * v + 1]; p[2] = X[3 * v + 2]; }
__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// one normal-consistency pair (v0, v1, a, b): n0 = e x (a - v0), n1 = -e x (b - v0), term 1 - cos(n0, n1) (torch.cosine_similarity: each
// vector divided by max(|n|, 1e-8)).  With gd != NULL, the gradient of the term at the pair's four vertices (v0, v1, a, b).
__device__ __forceinline__ float normal_pair(const float *X, int4 p, float (*gd)[3]) {
    float P0[3], P1[3], A[3], Bv[3];
    ld3(X, p.x, P0); ld3(X, p.y, P1); ld3(X, p.z, A); ld3(X, p.w, Bv);
    float e[3], u[3], w[3];
    for (int k = 0; k < 3; ++k) { e[k] = P1[k] - P0[k]; u[k] = A[k] - P0[k]; w[k] = Bv[k] - P0[k]; }
    float n0[3], n1[3];
    cross3(e, u, n0);
    cross3(e, w, n1);
    for (int k = 0; k < 3; ++k) n1[k] = -n1[k];
    const float l0 = fmaxf(sqrtf(dot3(n0, n0)), 1e-8f), l1 = fmaxf(sqrtf(dot3(n1, n1)), 1e-8f);
    float h0[3], h1[3];
    for (int k = 0; k < 3; ++k) { h0[k] = n0[k] / l0; h1[k] = n1[k] / l1; }
    const float c = dot3(h0, h1);
    if (gd) {
        // d(-cos)/dn0 = -(h1 - c h0) / l0, d(-cos)/dn1 = -(h0 - c h1) / l1
        float g0[3], g1[3];
        for (int k = 0; k < 3; ++k) { g0[k] = -(h1[k] - c * h0[k]) / l0; g1[k] = (h0[k] - c * h1[k]) / l1; }  // g1: through n1 = -(e x w)
        // n = e x u: de += u x g, du += g x e
        float ue[3], uu[3], we[3], ww[3];
        cross3(u, g0, ue); cross3(g0, e, uu);
        cross3(w, g1, we); cross3(g1, e, ww);
        for (int k = 0; k < 3; ++k) {
            const float de = ue[k] + we[k];
            gd[0][k] = -de - uu[k] - ww[k];
            gd[1][k] = de;
            gd[2][k] = uu[k];
            gd[3][k] = ww[k];
        }
    }
    return 1.0f - c;
}

// Laplacian residual of row i: (1/deg) sum_{j in N(i)} v_j - v_i, summed as (1/deg) sum (v_j - v_i): the neighbour differences are
// small and exact where the coordinates are not, so a short residual keeps its direction (which is its gradient).  Isolated: -v_i.
__device__ __forceinline__ void lap_row(const SmilMeshTopology &t, const float *X, int i, float (&r)[3]) {
    const int e0 = t.nbr_ptr[i], e1 = t.nbr_ptr[i + 1];
    if (e0 == e1) {
        for (int k = 0; k < 3; ++k) r[k] = -X[3 * i + k];
        return;
    }
    float s[3] = {0.f, 0.f, 0.f};
    for (int e = e0; e < e1; ++e) {
        const int j = t.nbr[e];
        for (int k = 0; k < 3; ++k) s[k] += X[3 * j + k] - X[3 * i + k];
    }
    const float id = t.inv_deg[i];
    for (int k = 0; k < 3; ++k) r[k] = s[k] * id;
}

__global__ void __launch_bounds__(REG_BLOCK) k_mesh_reg(RegArgs a) {
    __shared__ float red[16];
    const SmilMeshTopology &t = a.t;
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float *X = a.verts + (size_t)b * t.V * 3;
    const float invB = 1.0f / (float)a.B;
    float le = 0.f, ln = 0.f, ll = 0.f;
    if ((a.terms & SMIL_REG_EDGE) && i < t.E) {
        const int2 e = make_int2(t.edges[2 * i], t.edges[2 * i + 1]);
        float d[3];
        for (int k = 0; k < 3; ++k) d[k] = X[3 * e.x + k] - X[3 * e.y + k];
        le = dot3(d, d);
    }
    if ((a.terms & SMIL_REG_NORMAL) && i < t.Q) {
        const int4 p = make_int4(t.pairs[4 * i], t.pairs[4 * i + 1], t.pairs[4 * i + 2], t.pairs[4 * i + 3]);
        ln = normal_pair(X, p, nullptr);
    }
    if (i < t.V) {
        const size_t o = ((size_t)b * t.V + i) * 3;
        float r[3];
        if (a.terms & SMIL_REG_LAPLACIAN) {
            lap_row(t, X, i, r);
            ll = sqrtf(dot3(r, r));
        }
        if ((a.terms & SMIL_REG_EDGE) && a.d_edge) {  // sum over the edges at i of 2 (v_i - v_j) / E
            float g[3] = {0.f, 0.f, 0.f};
            for (int e = t.nbr_ptr[i]; e < t.nbr_ptr[i + 1]; ++e) {
                const int j = t.nbr[e];
                for (int k = 0; k < 3; ++k) g[k] += X[3 * i + k] - X[3 * j + k];
            }
            const float s = t.E > 0 ? 2.0f / (float)t.E * invB : 0.f;
            for (int k = 0; k < 3; ++k) a.d_edge[o + k] = g[k] * s;
        }
        if ((a.terms & SMIL_REG_LAPLACIAN) && a.d_lap) {  // -ghat_i + sum_{j in N(i)} ghat_j / deg_j, ghat = r / |r| (0 at |r| = 0)
            float g[3];
            const float inv = ll > 0.f ? 1.0f / ll : 0.f;
            for (int k = 0; k < 3; ++k) g[k] = -r[k] * inv;
            for (int e = t.nbr_ptr[i]; e < t.nbr_ptr[i + 1]; ++e) {
                const int j = t.nbr[e];
                float rj[3];
                lap_row(t, X, j, rj);
                const float nj = sqrtf(dot3(rj, rj));
                const float sj = nj > 0.f ? t.inv_deg[j] / nj : 0.f;
                for (int k = 0; k < 3; ++k) g[k] += rj[k] * sj;
            }
            const float s = 1.0f / (float)t.V * invB;
            for (int k = 0; k < 3; ++k) a.d_lap[o + k] = g[k] * s;
        }
        if ((a.terms & SMIL_REG_NORMAL) && a.d_normal) {
            float g[3] = {0.f, 0.f, 0.f};
            for (int e = t.vpair_ptr[i]; e < t.vpair_ptr[i + 1]; ++e) {
                const int code = t.vpair[e], q = code >> 2, role = code & 3;
                const int4 p = make_int4(t.pairs[4 * q], t.pairs[4 * q + 1], t.pairs[4 * q + 2], t.pairs[4 * q + 3]);
                float gd[4][3];
                normal_pair(X, p, gd);
                for (int k = 0; k < 3; ++k) g[k] += gd[role][k];
            }
            const float s = t.Q > 0 ? 1.0f / (float)t.Q * invB : 0.f;
            for (int k = 0; k < 3; ++k) a.d_normal[o + k] = g[k] * s;
        }
    }
    le = block_sum(le, red);
    ln = block_sum(ln, red);
    ll = block_sum(ll, red);
    if (threadIdx.x == 0) {
        float *p = a.part + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        p[0] = le; p[1] = ln; p[2] = ll;
    }
}

__global__ void __launch_bounds__(256) k_mesh_reg_reduce(RegArgs a, int nblk) {
    const SmilMeshTopology &t = a.t;
    const float cnt[3] = {(float)t.E, (float)t.Q, (float)t.V};
    for (int w = threadIdx.x; w < a.B * 3; w += blockDim.x) {
        const int b = w / 3, k = w % 3;
        float s = 0.f;
        for (int j = 0; j < nblk; ++j) s += a.part[((size_t)b * nblk + j) * 3 + k];
        a.per_mesh[w] = cnt[k] > 0.f ? s / cnt[k] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float s = 0.f;
        for (int b = 0; b < a.B; ++b) s += a.per_mesh[b * 3 + threadIdx.x];
        a.out[threadIdx.x] = s / (float)a.B;
    }
}

static int reg_blocks(const SmilMeshTopology *t) { return ceil_div(std::max(std::max(t->V, t->E), std::max(t->Q, 1)), REG_BLOCK); }

static size_t reg_layout(const SmilMeshTopology *t, int B, char *base, RegArgs &a) {
    Workspace w{base};
    a.part = w.take<float>((size_t)B * reg_blocks(t) * 3);
    a.per_mesh = w.take<float>((size_t)B * 3);
    return w.used;
}

extern "C" size_t smil_mesh_reg_workspace_bytes(const SmilMeshTopology *t, int32_t B) {
    RegArgs a;
    return (t && B > 0 && t->V > 0) ? reg_layout(t, B, nullptr, a) : 0;
}

extern "C" int smil_mesh_regularisers(const SmilMeshTopology *t, const float *verts, int32_t B, int32_t terms, float *out3, float *d_edge,
                                      float *d_normal, float *d_lap, void *workspace, void *stream_) {
    SMIL_REQUIRE(t && verts && out3 && workspace, "smil_mesh_regularisers: null argument");
    SMIL_REQUIRE(B > 0 && B <= 65535 && t->V > 0 && t->E >= 0 && t->Q >= 0, "smil_mesh_regularisers: bad sizes B=%d V=%d E=%d Q=%d", B, t->V,
                 t->E, t->Q);
    SMIL_REQUIRE(terms > 0 && (terms & ~(SMIL_REG_EDGE | SMIL_REG_NORMAL | SMIL_REG_LAPLACIAN)) == 0, "smil_mesh_regularisers: bad terms mask %d",
                 terms);
    SMIL_REQUIRE(t->nbr_ptr && t->inv_deg && (t->E == 0 || (t->edges && t->nbr)) && (t->Q == 0 || (t->pairs && t->vpair && t->vpair_ptr)),
                 "smil_mesh_regularisers: topology tables missing");
    SMIL_REQUIRE(t->vpair_ptr || !(terms & SMIL_REG_NORMAL) || !d_normal, "smil_mesh_regularisers: vertex -> pair table missing");
    hipStream_t stream = (hipStream_t)stream_;
    RegArgs a;
    a.t = *t;
    a.verts = verts; a.B = B; a.terms = terms;
    a.d_edge = d_edge; a.d_normal = d_normal; a.d_lap = d_lap;
    const int nblk = reg_blocks(t);
    reg_layout(t, B, (char *)workspace, a);
    a.out = out3;
    hipLaunchKernelGGL(k_mesh_reg, dim3(nblk, B), dim3(REG_BLOCK), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_reg_reduce, dim3(1), dim3(256), 0, stream, a, nblk);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---------------------------------------------------------------------------------------------
// K nearest neighbours (pytorch3d.ops.knn_points, norm 2, no lengths)
// ---------------------------------------------------------------------------------------------
#define KNN_BLOCK 256
#define KNN_QPW 4                     // queries per wave of k_knn
#define KNN_QPB (KNN_QPW * KNN_BLOCK / WAVE)
#define KNN_TILE 256                  // candidates staged in LDS per step
#define KNN_EMPTY SCAN_KEY_NONE
static_assert(SMIL_KNN_MAX_K == WAVE, "k_knn keeps one list entry per lane");

struct KnnArgs {
    const float *pts[2];           // (N, P[d], 3): direction d's queries are pts[d], its candidates pts[1 - d]
    int P[2];
    int N, dirs, K;
    float *dists[2];               // (N, P[d], K) ascending by (distance, candidate index)
    int *idx[2];                   // (N, P[d], K)
    unsigned int *dmax;            // (N, 2) bits of the largest K-th distance of (mesh, direction), or NULL
    unsigned long long *n_insert;  // (1) list insertions of the call, or NULL
};

// Lane l of a wave holds the l-th smallest key seen so far of each of the wave's KNN_QPW queries (KNN_EMPTY: none yet); keys order
// like (distance, index) because distances are >= 0.  All 64 entries are kept whatever K is: thr, the key of lane K - 1, is what a
// candidate has to beat, and the first K lanes are the result.  A step gives every lane one candidate; the lanes whose candidate
// beats thr are served in lane order (ascending index), each tested again because thr falls with every insertion, and an
// insertion is one shift by a lane of the entries above the new key.  No list is indexed at run time: nothing goes to scratch.
__global__ void __launch_bounds__(KNN_BLOCK) k_knn(KnnArgs a) {
    __shared__ float4 tile[KNN_TILE];
    const int d = blockIdx.z % a.dirs, n = blockIdx.z / a.dirs;
    const int Pq = a.P[d], Pc = a.P[1 - d];
    if ((int)blockIdx.x * KNN_QPB >= Pq) return;  // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const int q0 = ((int)blockIdx.x * (KNN_BLOCK / WAVE) + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)) * KNN_QPW;
    const float *Q = a.pts[d] + (size_t)n * Pq * 3;
    const float *C = a.pts[1 - d] + (size_t)n * Pc * 3;
    float qx[KNN_QPW], qy[KNN_QPW], qz[KNN_QPW];
    unsigned long long key[KNN_QPW], thr[KNN_QPW];
#pragma unroll
    for (int k = 0; k < KNN_QPW; ++k) {
        const int qc = min(q0 + k, Pq - 1);
        qx[k] = Q[3 * qc]; qy[k] = Q[3 * qc + 1]; qz[k] = Q[3 * qc + 2];
        key[k] = KNN_EMPTY;
        thr[k] = q0 + k < Pq ? KNN_EMPTY : 0ull;  // (a query past the end accepts nothing)
    }
    unsigned int ins = 0;
    scan_tiles<KNN_TILE>(0, Pc, tile, ScanStageXyz{C}, [&](int c0, int cnt) {
        for (int j0 = 0; j0 < cnt; j0 += WAVE) {
            const int j = j0 + lane;  // (< KNN_TILE: the read stays inside the tile, entries past cnt are not used)
            const float4 c = tile[j];
#pragma unroll
            for (int k = 0; k < KNN_QPW; ++k) {
                const float dx = qx[k] - c.x, dy = qy[k] - c.y, dz = qz[k] - c.z;
                const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                const unsigned long long ck = j < cnt ? scan_key(dd, c0 + j) : KNN_EMPTY;
                unsigned long long m = __ballot(ck < thr[k]);
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const unsigned long long nk = read_lane(ck, l);
                    if (nk < thr[k]) {
                        const unsigned long long up = __shfl_up(key[k], 1, WAVE);
                        if (key[k] > nk) key[k] = (lane > 0 && up > nk) ? up : nk;
                        thr[k] = read_lane(key[k], a.K - 1);
                        ++ins;
                    }
                }
            }
        }
    });
    float kmax = 0.f;
#pragma unroll
    for (int k = 0; k < KNN_QPW; ++k) {
        const int q = q0 + k;
        if (q < Pq) {
            if (lane < a.K) {
                const size_t o = ((size_t)n * Pq + q) * a.K + lane;
                a.dists[d][o] = scan_key_value(key[k]);
                a.idx[d][o] = scan_key_index(key[k]);
            }
            kmax = fmaxf(kmax, scan_key_value(thr[k]));  // (K <= Pc: the K-th entry is a candidate)
        }
    }
    if (lane == 0) {  // (kmax is wave-uniform already: fix_record_max's wave maximum is not needed; the sum is an integer's)
        if (a.dmax) atomicMax(&a.dmax[n * 2 + d], __float_as_uint(kmax));
        if (a.n_insert) atomicAdd(a.n_insert, (unsigned long long)ins);
    }
}

static bool knn_sizes_ok(int N, int P1, int P2, int K, bool both) {
    return N > 0 && P1 > 0 && P2 > 0 && K >= 1 && K <= SMIL_KNN_MAX_K && K <= P2 && (!both || K <= P1) && N <= 32767 &&
           (size_t)std::max(P1, P2) * (size_t)K <= 0x7FFFFFFFu;
}

static size_t knn_layout(char *base, KnnArgs &a) {
    Workspace w{base};
    a.n_insert = w.take<unsigned long long>(1);
    return w.used;
}

extern "C" size_t smil_knn_workspace_bytes(int32_t N, int32_t P1, int32_t P2, int32_t K) {
    KnnArgs a;
    return knn_sizes_ok(N, P1, P2, K, false) ? knn_layout(nullptr, a) : 0;
}

static int knn_launch(KnnArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(k_knn, dim3(ceil_div(std::max(a.P[0], a.dirs == 2 ? a.P[1] : 1), KNN_QPB), 1, a.N * a.dirs), dim3(KNN_BLOCK), 0, stream,
                       a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_knn(const float *x, const float *y, int32_t N, int32_t P1, int32_t P2, int32_t K, float *dists_x, int32_t *idx_x,
                        float *dists_y, int32_t *idx_y, void *workspace, void *stream_) {
    SMIL_REQUIRE(x && y && dists_x && idx_x && workspace, "smil_knn: null argument");
    SMIL_REQUIRE((dists_y == nullptr) == (idx_y == nullptr), "smil_knn: dists_y and idx_y are given together or not at all");
    SMIL_REQUIRE(knn_sizes_ok(N, P1, P2, K, dists_y != nullptr),
                 "smil_knn: bad sizes N=%d P1=%d P2=%d K=%d (1 <= K <= %d, K <= candidates, N <= 32767)", N, P1, P2, K, SMIL_KNN_MAX_K);
    hipStream_t stream = (hipStream_t)stream_;
    KnnArgs a;
    knn_layout((char *)workspace, a);
    a.pts[0] = x; a.pts[1] = y;
    a.P[0] = P1; a.P[1] = P2;
    a.N = N; a.dirs = dists_y ? 2 : 1; a.K = K;
    a.dists[0] = dists_x; a.dists[1] = dists_y;
    a.idx[0] = (int *)idx_x; a.idx[1] = (int *)idx_y;
    a.dmax = nullptr;
    SMIL_HIP(hipMemsetAsync(a.n_insert, 0, sizeof(unsigned long long), stream));
    return knn_launch(a, stream);
}

// ---------------------------------------------------------------------------------------------
// the SDF-guided term (reference fitter_3d/utils.py:973-1261)
// ---------------------------------------------------------------------------------------------
#define SDF_INV_TEMPERATURE 10.0  // utils.py:1069: temperature 0.1
#define SDF_STD_MIN 1e-8          // utils.py:1044

struct SdfArgs {
    CloudLossArgs c;       // clouds, weights, fixed-point accumulators, gradients, partial sums; c.dist holds r_i
    KnnArgs knn;
    const float *val[2];   // (N, P[s]) per-point values of side s
    double *z;             // (N, P[0] + P[1]) their z-scores, side 0's first (ch_row)
};

// sums of blockDim.x = 256 doubles in a fixed order; the result in every thread
__device__ __forceinline__ double block_sum_f64(double v, double *sm) {
    __syncthreads();
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    return sm[0];
}

// z = (s - mean) / max(std, 1e-8) per (mesh, side), std unbiased (torch's default): the mean first, then the squares of the
// differences from it, both in float64, so a large common offset of the values costs nothing.
__global__ void __launch_bounds__(256) k_sdf_stats(SdfArgs a) {
    __shared__ double sm[256];
    const int side = blockIdx.x & 1, n = blockIdx.x >> 1;
    const int P = a.c.P[side];
    const float *v = a.val[side] + (size_t)n * P;
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) s += (double)v[i];
    const double mean = block_sum_f64(s, sm) / (double)P;
    double ss = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) {
        const double e = (double)v[i] - mean;
        ss += e * e;
    }
    const double sd = fmax(sqrt(block_sum_f64(ss, sm) / (double)(P - 1)), SDF_STD_MIN);
    double *z = a.z + ch_row(a.c, n, side);
    for (int i = threadIdx.x; i < P; i += 256) z[i] = ((double)v[i] - mean) / sd;
}

// wave = one query i of direction d, lane k = its k-th neighbour j: w_k = softmax_k(-|z_q[i] - z_c[j]| / 0.1), r_i = sum_k w_k d_k,
// the owned gradient 2 w sum_k w_k (q - c_j), and -w_k (q - c_j) added to candidate j's fixed-point sums.
__global__ void __launch_bounds__(256) k_sdf_term(SdfArgs a) {
    const int d = blockIdx.z % a.c.dirs, n = blockIdx.z / a.c.dirs;
    const int Pq = a.c.P[d], Pc = a.c.P[1 - d], K = a.knn.K;
    const int q = (int)blockIdx.x * (256 / WAVE) + ((int)threadIdx.x >> 6);
    if (q >= Pq) return;  // (wave-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const bool on = lane < K;
    const size_t row = ch_row(a.c, n, d) + q;
    const size_t o = ((size_t)n * Pq + q) * K + lane;
    int j = on ? a.knn.idx[d][o] : 0;
    const float dd = on ? a.knn.dists[d][o] : 0.f;
    j = min(max(j, 0), Pc - 1);
    const double zd = fabs(a.z[row] - a.z[ch_row(a.c, n, 1 - d) + j]) * SDF_INV_TEMPERATURE;
    const double lo = on ? -zd : -__builtin_inf();
    const double top = wave_max(lo);
    const float e = on ? expf((float)(lo - top)) : 0.f;
    const float w = e / wave_sum(e);
    const float r = wave_sum(w * dd);
    if (lane == 0) a.c.dist[row] = r;
    if (!a.c.grad[0]) return;
    const float *Qp = a.c.pts[d] + ((size_t)n * Pq + q) * 3;
    const float *Cp = a.c.pts[1 - d] + ((size_t)n * Pc + j) * 3;
    const float ex[3] = {Qp[0] - Cp[0], Qp[1] - Cp[1], Qp[2] - Cp[2]};
    const float s = 2.0f * a.c.w[d];
    const float g0 = wave_sum(w * ex[0]), g1 = wave_sum(w * ex[1]), g2 = wave_sum(w * ex[2]);
    if (lane == 0) {
        float *g = a.c.grad[d] + ((size_t)n * Pq + q) * 3;
        g[0] = s * g0; g[1] = s * g1; g[2] = s * g2;
    }
    if (on) {  // (the product in float64 is exact: the integer added does not depend on the clouds' scale)
        long long *acc = a.c.acc + (ch_row(a.c, n, 1 - d) + j) * 3;
        const int fix = ch_fix_exp(a.c, n, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(&acc[k], -(double)w * (double)ex[k], fix);
    }
}

static bool sdf_sizes_ok(int N, int P1, int P2, int K, bool both) { return knn_sizes_ok(N, P1, P2, K, both) && P1 >= 2 && P2 >= 2; }

static size_t sdf_layout(int N, int P1, int P2, int K, bool own_tables, char *base, SdfArgs &a) {
    const size_t pts = (size_t)N * ((size_t)P1 + P2);
    Workspace w{base};
    a.knn.n_insert = w.take<unsigned long long>(1);
    a.c.dmax = w.take<unsigned int>((size_t)N * 2);
    a.c.part = w.take<float>((size_t)N * 2);
    a.c.dist = w.take<float>(pts);
    a.z = w.take<double>(pts);
    a.c.acc = w.take<long long>(pts * 3);
    if (own_tables) {
        a.knn.dists[0] = w.take<float>((size_t)N * P1 * K);
        a.knn.idx[0] = w.take<int>((size_t)N * P1 * K);
        a.knn.dists[1] = w.take<float>((size_t)N * P2 * K);
        a.knn.idx[1] = w.take<int>((size_t)N * P2 * K);
    }
    return w.used;
}

extern "C" size_t smil_sdf_distance_workspace_bytes(int32_t N, int32_t P1, int32_t P2, int32_t K) {
    SdfArgs a;
    return sdf_sizes_ok(N, P1, P2, K, false) ? sdf_layout(N, P1, P2, K, true, nullptr, a) : 0;
}

extern "C" int smil_sdf_distance(const float *x, const float *y, const float *x_sdf, const float *y_sdf, int32_t N, int32_t P1, int32_t P2,
                                 int32_t K, int32_t single_directional, int32_t point_sum, int32_t batch_sum, float *loss, float *d_x,
                                 float *d_y, float *dists_x, int32_t *idx_x, float *dists_y, int32_t *idx_y, void *workspace,
                                 void *stream_) {
    SMIL_REQUIRE(x && y && x_sdf && y_sdf && loss && workspace, "smil_sdf_distance: null argument");
    SMIL_REQUIRE(sdf_sizes_ok(N, P1, P2, K, !single_directional),
                 "smil_sdf_distance: bad sizes N=%d P1=%d P2=%d K=%d (1 <= K <= %d, K <= candidates, P >= 2, N <= 32767)", N, P1, P2, K,
                 SMIL_KNN_MAX_K);
    SMIL_REQUIRE((d_x == nullptr) == (d_y == nullptr), "smil_sdf_distance: d_x and d_y are given together or not at all");
    SMIL_REQUIRE((dists_x == nullptr) == (idx_x == nullptr) && (dists_y == nullptr) == (idx_y == nullptr),
                 "smil_sdf_distance: a neighbour table is its dists and its idx");
    SMIL_REQUIRE(!(single_directional && dists_y), "smil_sdf_distance: dists_y has no meaning when single_directional");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t pts = (size_t)N * ((size_t)P1 + P2);
    SdfArgs a;
    sdf_layout(N, P1, P2, K, true, (char *)workspace, a);
    if (dists_x) { a.knn.dists[0] = dists_x; a.knn.idx[0] = (int *)idx_x; }
    if (dists_y) { a.knn.dists[1] = dists_y; a.knn.idx[1] = (int *)idx_y; }
    CloudLossArgs &c = a.c;
    cloud_loss_fill(c, x, y, N, P1, P2, single_directional, point_sum, batch_sum, d_x, d_y, loss);
    c.K = K;
    a.knn.pts[0] = x; a.knn.pts[1] = y;
    a.knn.P[0] = P1; a.knn.P[1] = P2;
    a.knn.N = N; a.knn.dirs = c.dirs; a.knn.K = K;
    a.knn.dmax = c.dmax;
    a.val[0] = x_sdf; a.val[1] = y_sdf;
    SMIL_HIP(hipMemsetAsync(a.knn.n_insert, 0, sizeof(unsigned long long), stream));
    SMIL_HIP(hipMemsetAsync(c.dmax, 0, (size_t)N * 2 * sizeof(unsigned int), stream));
    if (d_x) SMIL_HIP(hipMemsetAsync(c.acc, 0, pts * 3 * 8, stream));
    hipLaunchKernelGGL(k_sdf_stats, dim3(N * 2), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    if (knn_launch(a.knn, stream) != SMIL_OK) return SMIL_E_DEVICE;
    hipLaunchKernelGGL(k_sdf_term, dim3(ceil_div(std::max(P1, c.dirs == 2 ? P2 : 1), 256 / WAVE), 1, N * c.dirs), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return cloud_loss_finish(c, stream);
}

// ---------------------------------------------------------------------------------------------
// vertex sampling (reference fitter_3d/utils.py:1264-1394)
// ---------------------------------------------------------------------------------------------
#define SV_STREAM 1u  // third counter word: the surface sampler's draws use 0

__global__ void __launch_bounds__(256) k_sample_vertices(const float *__restrict__ verts, const float *__restrict__ values,
                                                         const int *__restrict__ vert_off, int S, uint32_t seed_lo, uint32_t seed_hi,
                                                         float *__restrict__ out, float *__restrict__ out_val, int *__restrict__ out_idx) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = blockIdx.y;
    if (s >= S) return;
    const size_t o = (size_t)n * S + s;
    const int v0 = vert_off[n], V = vert_off[n + 1] - v0;
    if (V <= 0) {  // an empty mesh: zeros, as the reference leaves them
        out[3 * o] = 0.f; out[3 * o + 1] = 0.f; out[3 * o + 2] = 0.f;
        out_val[o] = 0.f;
        out_idx[o] = -1;
        return;
    }
    const uint4 r = philox4x32_10(make_uint4((uint32_t)s, (uint32_t)n, SV_STREAM, 0u), make_uint2(seed_lo, seed_hi));
    const int i = (int)(((uint64_t)r.x * (uint64_t)(uint32_t)V) >> 32);  // [0, V)
    const float *p = verts + 3 * (size_t)(v0 + i);
    out[3 * o] = p[0]; out[3 * o + 1] = p[1]; out[3 * o + 2] = p[2];
    out_val[o] = values[v0 + i];
    out_idx[o] = i;
}

extern "C" int smil_sample_vertices(const float *verts, const float *values, const int32_t *vert_off, int32_t N, int32_t S, uint64_t seed,
                                    float *out, float *out_values, int32_t *out_idx, void *stream_) {
    SMIL_REQUIRE(verts && values && vert_off && out && out_values && out_idx, "smil_sample_vertices: null argument");
    SMIL_REQUIRE(N > 0 && S > 0 && N <= 65535, "smil_sample_vertices: bad sizes N=%d S=%d (N <= 65535)", N, S);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_sample_vertices, dim3(ceil_div(S, 256), N), dim3(256), 0, stream, verts, values, (const int *)vert_off, S,
                       (uint32_t)seed, (uint32_t)(seed >> 32), out, out_values, (int *)out_idx);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// The gradient of the sampled points back to the vertices: duplicates of a vertex are summed as int64 fixed point (common.h);
// magnitude: the mesh's largest |component|, addends: S.
struct SvGradArgs {
    const float *d_pts;    // (N, S, 3)
    const int *idx;        // (N, S) vertex within its mesh, -1: none
    const int *vert_off;   // (N + 1)
    int N, S;
    float *d_verts;        // (n_verts, 3)
    long long *acc;        // (n_verts, 3)
    unsigned int *gmax;    // (N) bits of the mesh's largest |component|
};

__device__ __forceinline__ int sv_fix_exp(const SvGradArgs &a, int n) { return fix_unit_exp(fix_max_exp(a.gmax[n]), (unsigned)a.S); }

__global__ void __launch_bounds__(256) k_sv_max(SvGradArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    float m = 0.f;
    if (s < a.S) {
        const float *g = a.d_pts + ((size_t)n * a.S + s) * 3;
        m = fmaxf(fabsf(g[0]), fmaxf(fabsf(g[1]), fabsf(g[2])));
    }
    fix_record_max(&a.gmax[n], m);
}

__global__ void __launch_bounds__(256) k_sv_add(SvGradArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (s >= a.S) return;
    const size_t o = (size_t)n * a.S + s;
    const int v0 = a.vert_off[n], i = a.idx[o];
    if (i < 0 || i >= a.vert_off[n + 1] - v0) return;
    const int fix = sv_fix_exp(a, n);
    long long *acc = a.acc + (size_t)(v0 + i) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) fix_add(&acc[k], (double)a.d_pts[3 * o + k], fix);
}

__global__ void __launch_bounds__(256) k_sv_out(SvGradArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    const int v0 = a.vert_off[n];
    if (i >= a.vert_off[n + 1] - v0) return;
    const int fix = sv_fix_exp(a, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.d_verts[(size_t)(v0 + i) * 3 + k] = fix_read(a.acc[(size_t)(v0 + i) * 3 + k], fix);
}

static size_t sv_grad_layout(int n_verts, int N, char *base, SvGradArgs &a) {
    Workspace w{base};
    a.acc = w.take<long long>((size_t)n_verts * 3);
    a.gmax = w.take<unsigned int>((size_t)N);
    return w.used;
}

extern "C" size_t smil_sample_vertices_backward_workspace_bytes(int32_t n_verts, int32_t N) {
    SvGradArgs a;
    return (n_verts > 0 && N > 0) ? sv_grad_layout(n_verts, N, nullptr, a) : 0;
}

extern "C" int smil_sample_vertices_backward(const float *d_pts, const int32_t *idx, const int32_t *vert_off, int32_t n_verts, int32_t max_verts,
                                             int32_t N, int32_t S, float *d_verts, void *workspace, void *stream_) {
    SMIL_REQUIRE(d_pts && idx && vert_off && d_verts && workspace, "smil_sample_vertices_backward: null argument");
    SMIL_REQUIRE(N > 0 && S > 0 && N <= 65535 && n_verts > 0 && max_verts > 0 && max_verts <= n_verts,
                 "smil_sample_vertices_backward: bad sizes N=%d S=%d n_verts=%d max_verts=%d", N, S, n_verts, max_verts);
    hipStream_t stream = (hipStream_t)stream_;
    SvGradArgs a;
    sv_grad_layout(n_verts, N, (char *)workspace, a);
    a.d_pts = d_pts; a.idx = (const int *)idx; a.vert_off = (const int *)vert_off;
    a.N = N; a.S = S; a.d_verts = d_verts;
    SMIL_HIP(hipMemsetAsync(a.acc, 0, (size_t)n_verts * 3 * 8, stream));
    SMIL_HIP(hipMemsetAsync(a.gmax, 0, (size_t)N * sizeof(unsigned int), stream));
    SMIL_HIP(hipMemsetAsync(d_verts, 0, (size_t)n_verts * 3 * sizeof(float), stream));  // (vertices outside vert_off's ranges)
    hipLaunchKernelGGL(k_sv_max, dim3(ceil_div(S, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sv_add, dim3(ceil_div(S, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sv_out, dim3(ceil_div(max_verts, 256), N), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
