// Multi-view visual hulls from silhouette masks (voxel carving) for gfx950.  The specification is at include/smilfit.h ("Visual hull").
//
// Conventions, restated once.  Camera arithmetic is that of smil_kp2d_fit_eval (joints.hip), float64 on the float32 SmilCameras tables:
// X_view = X R + T; k11 = 1 / tan(fov / 2) (degrees), k00 = k11 / aspect; x_ndc = k00 x / z + px, y_ndc = k11 y / z + py (the principal
// point added after the division); y_s = S/2 - (S/2) y_ndc, x_s likewise.  Tables of 1, views or N views rows are indexed image % rows,
// image = frame views + view.  Pixel (r, c) of an H x W mask covers [r, r+1) x [c, c+1) in (y_s, x_s) (pix_to_ndc, common.h: pixel
// centres at + 0.5); the mask need not be square or of side S.  A view SEES a point iff z_view > SMIL_ZNEAR, 0 <= y_s < H and
// 0 <= x_s < W, decided in floating point before any conversion to an integer: a NaN or infinite coordinate fails every comparison and
// never becomes an index.  A seen point is foreground iff the mask value is > threshold (a float NaN is not).
//
//  * hull_votes        the projection and lookup of ONE point in every view of its frame: what the carve and the query share.  The
//                      frame's cameras are staged in LDS as (views,16) float64 (every lane reads the same row: a broadcast).  The mask
//                      tap of a view that does not see the point is LOADED from the view's pixel (0,0) and discarded: a load under a
//                      per-lane condition is a branch with a wait of its own (imageprep.hip, k_warp), and with the loop unrolled by
//                      four, four taps are in flight.
//  * k_hull_carve      one lane per voxel, HULL_VOX voxels per thread a block apart, consecutive lanes on consecutive x: the byte
//                      stores are coalesced and neighbouring voxels tap neighbouring pixels.  Voxel centres are formed with
//                      contraction off (origin + (i + 0.5) voxel_size: three roundings, specified to the bit - the surface points
//                      are these numbers rounded once).  A pure gather: no atomics, bit-reproducible by construction.
//  * k_hull_query      the same for arbitrary float32 points.
//  * k_hull_stats      exact int64 sums, minima and maxima of the occupied voxel indices: per-thread, wave butterfly (common.h), LDS across the
//                      waves, then one set of integer atomics per block into a row that k_hull_stats_init has preset.  Integer sums,
//                      minima and maxima do not depend on the order.
//  * k_hull_surface<WRITE>  a block looks at HULL_SURF_VOX consecutive voxels per thread.  WRITE false: its count of surface voxels
//                      into the workspace; k_hull_scan turns the counts into exclusive prefixes and the frames' offsets.
//                      WRITE true: the same flags again, a block-wide exclusive scan of the threads' counts (block_scan_exclusive,
//                      hull_grid.h), and every surface voxel stored at prefix of its block + prefix of its thread + its rank in the
//                      thread: ascending linear voxel index, whatever the scheduling.
//  * k_hull_scan       the ONE scan of per-workgroup counts, launched through hull_scan (hull_grid.h) by the surface count here (one
//                      job) and by the mesh count of hull_mesh.hip (two jobs: vertices, and quads scaled to triangles).  A workgroup
//                      per job scans 1 024 counts a round with block_scan_exclusive and carries the rounds' totals.
// Every voxel index is 64-bit (N Gx Gy Gz may exceed 2^31; a frame whose own count stays below 2^31 decodes (i, j, k) with 32-bit
// divisions, a wave-uniform choice).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "hull_grid.h"

#define HULL_STAT_VOX 16  // voxels per thread of the statistics, HULL_THREADS apart
#define HULL_CAM 16       // doubles of a staged camera

// (joints.hip, stage_camera64, restated: that file's kernels are pinned to their instructions and share no header with this one)
__device__ __forceinline__ void hull_stage_camera(double *row, const SmilCameras &c, int n) {
    const float *R = c.R + (size_t)(n % c.nR) * 9, *T = c.T + (size_t)(n % c.nT) * 3;
    for (int i = 0; i < 9; ++i) row[i] = (double)R[i];
    for (int i = 0; i < 3; ++i) row[9 + i] = (double)T[i];
    const double k11 = 1.0 / tan((double)c.fov[n % c.nFov] * 0.017453292519943295 / 2.0);
    row[12] = c.aspect ? k11 / (double)c.aspect[n % c.nAspect] : k11;
    row[13] = k11;
    row[14] = c.principal ? (double)c.principal[2 * (size_t)(n % c.nPrincipal)] : 0.0;
    row[15] = c.principal ? (double)c.principal[2 * (size_t)(n % c.nPrincipal) + 1] : 0.0;
}

struct HullLookup {
    const void *masks;  // (N, views, H, W)
    SmilCameras cam;
    int H, W;
    float threshold;
    int outside_carves;
};

__device__ __forceinline__ void hull_stage_frame(double *sCam, const HullLookup &a, long long frame) {
    for (int v = threadIdx.x; v < a.cam.views; v += blockDim.x) hull_stage_camera(sCam + HULL_CAM * v, a.cam, (int)(frame * a.cam.views + v));
    __syncthreads();
}

// fg, seen of the point (X, Y, Z) over the views of a frame whose first mask is `masks`
template <typename T>
__device__ __forceinline__ void hull_votes(const double *sCam, const HullLookup &a, const T *masks, double X, double Y, double Z, int &fg,
                                           int &seen) {
    const double hS = 0.5 * (double)a.cam.S, dH = (double)a.H, dW = (double)a.W;
    const size_t plane = (size_t)a.H * a.W;
    int f = 0, s = 0;
#pragma unroll 4
    for (int v = 0; v < a.cam.views; ++v) {
        const double *cm = sCam + HULL_CAM * v;
        const double vx = X * cm[0] + Y * cm[3] + Z * cm[6] + cm[9];
        const double vy = X * cm[1] + Y * cm[4] + Z * cm[7] + cm[10];
        const double vz = X * cm[2] + Y * cm[5] + Z * cm[8] + cm[11];
        const bool front = vz > (double)SMIL_ZNEAR;
        const double iz = 1.0 / vz;
        const double xn = vx * cm[12] * iz, yn = vy * cm[13] * iz;
        const double ys = hS - hS * (yn + cm[15]), xs = hS - hS * (xn + cm[14]);
        const bool in = front && ys >= 0.0 && ys < dH && xs >= 0.0 && xs < dW;  // (false for a NaN or an infinity)
        const int r = in ? (int)ys : 0, c = in ? (int)xs : 0;                   // 0 <= ys < H: the conversion is floor
        const T m = masks[(size_t)v * plane + (size_t)r * a.W + c];
        f += (in && (float)m > a.threshold) ? 1 : 0;
        s += (a.outside_carves ? front : in) ? 1 : 0;
    }
    fg = f; seen = s;
}

// the centre of voxel i of an axis: three roundings, no fused multiply-add
__device__ __forceinline__ double hull_centre(double origin, long long i, double voxel) {
#pragma clang fp contract(off)
    const double t = ((double)i + 0.5) * voxel;
    return origin + t;
}

// linear voxel index of a frame -> (i, j, k), x fastest; `small`: the frame holds fewer than 2^31 voxels
__device__ __forceinline__ void hull_decode(long long v, int Gx, int Gy, bool small, int &i, int &j, int &k) {
    if (small) {
        const unsigned u = (unsigned)v, t = u / (unsigned)Gx, q = t / (unsigned)Gy;
        i = (int)(u - t * (unsigned)Gx); j = (int)(t - q * (unsigned)Gy); k = (int)q;
    } else {
        const long long t = v / Gx, q = t / Gy;
        i = (int)(v - t * Gx); j = (int)(t - q * Gy); k = (int)q;
    }
}

// ---- carve ------------------------------------------------------------------------------------------------------------------
struct CarveArgs {
    HullLookup look;
    HullGridDev g;
    int min_views, max_misses;
    unsigned char *occ, *fg, *seen;
};

template <typename T>
__global__ void __launch_bounds__(HULL_THREADS) k_hull_carve(CarveArgs a) {
    __shared__ double sCam[SMIL_HULL_MAX_VIEWS * HULL_CAM];
    const long long frame = (long long)(blockIdx.x / (unsigned long long)a.g.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)a.g.chunks);
    hull_stage_frame(sCam, a.look, frame);
    const double *org = a.g.origin + 3 * (frame % a.g.n_origin);
    const double voxel = a.g.voxel[frame % a.g.n_voxel];
    const T *masks = (const T *)a.look.masks + (size_t)frame * a.look.cam.views * ((size_t)a.look.H * a.look.W);
    const bool small = a.g.vox <= 0x7FFFFFFFLL;
#pragma unroll 1
    for (int q = 0; q < HULL_VOX; ++q) {
        const long long v = (chunk * HULL_VOX + q) * HULL_THREADS + threadIdx.x;
        if (v >= a.g.vox) break;  // (no barrier below)
        int i, j, k;
        hull_decode(v, a.g.Gx, a.g.Gy, small, i, j, k);
        int fg, seen;
        hull_votes<T>(sCam, a.look, masks, hull_centre(org[0], i, voxel), hull_centre(org[1], j, voxel), hull_centre(org[2], k, voxel), fg, seen);
        const size_t o = (size_t)frame * (size_t)a.g.vox + (size_t)v;
        a.occ[o] = (seen >= a.min_views && seen - fg <= a.max_misses) ? 1 : 0;
        if (a.fg) a.fg[o] = (unsigned char)fg;
        if (a.seen) a.seen[o] = (unsigned char)seen;
    }
}

// ---- query ------------------------------------------------------------------------------------------------------------------
struct QueryArgs {
    HullLookup look;
    const float *points;  // (N,P,3)
    long long P, chunks;
    unsigned char *fg, *seen;
};

template <typename T>
__global__ void __launch_bounds__(HULL_THREADS) k_hull_query(QueryArgs a) {
    __shared__ double sCam[SMIL_HULL_MAX_VIEWS * HULL_CAM];
    const long long frame = (long long)(blockIdx.x / (unsigned long long)a.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)a.chunks);
    hull_stage_frame(sCam, a.look, frame);
    const long long p = chunk * HULL_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const size_t o = (size_t)frame * (size_t)a.P + (size_t)p;
    const T *masks = (const T *)a.look.masks + (size_t)frame * a.look.cam.views * ((size_t)a.look.H * a.look.W);
    int fg, seen;
    hull_votes<T>(sCam, a.look, masks, (double)a.points[3 * o], (double)a.points[3 * o + 1], (double)a.points[3 * o + 2], fg, seen);
    a.fg[o] = (unsigned char)fg;
    a.seen[o] = (unsigned char)seen;
}

// ---- statistics -------------------------------------------------------------------------------------------------------------
__global__ void k_hull_stats_init(long long *stats, int N, int Gx, int Gy, int Gz) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    long long *s = stats + SMIL_HULL_STATS * (size_t)n;
    for (int c = 0; c < 10; ++c) s[c] = 0;
    s[10] = Gx; s[11] = Gy; s[12] = Gz;
    s[13] = s[14] = s[15] = -1;
}

__global__ void __launch_bounds__(HULL_THREADS) k_hull_stats(const unsigned char *occ, HullGridDev g, long long *stats) {
    __shared__ long long s_red[HULL_THREADS / 64][SMIL_HULL_STATS];
    const long long frame = (long long)(blockIdx.x / (unsigned long long)g.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)g.chunks);
    const unsigned char *o = occ + (size_t)frame * (size_t)g.vox;
    const bool small = g.vox <= 0x7FFFFFFFLL;
    long long a[SMIL_HULL_STATS];
#pragma unroll
    for (int c = 0; c < 10; ++c) a[c] = 0;
    a[10] = g.Gx; a[11] = g.Gy; a[12] = g.Gz;
    a[13] = a[14] = a[15] = -1;
    const long long v0 = chunk * (HULL_STAT_VOX * HULL_THREADS) + threadIdx.x;
    unsigned char b[HULL_STAT_VOX];
#pragma unroll
    for (int q = 0; q < HULL_STAT_VOX; ++q) {  // every byte loaded (the frame's last one again behind its end) before any is looked at
        const long long v = v0 + (long long)q * HULL_THREADS;
        b[q] = o[v < g.vox ? v : g.vox - 1];
    }
#pragma unroll
    for (int q = 0; q < HULL_STAT_VOX; ++q) {
        const long long v = v0 + (long long)q * HULL_THREADS;
        if (v >= g.vox || !b[q]) continue;
        int i, j, k;
        hull_decode(v, g.Gx, g.Gy, small, i, j, k);
        const long long li = i, lj = j, lk = k;
        a[0] += 1; a[1] += li; a[2] += lj; a[3] += lk;
        a[4] += li * li; a[5] += lj * lj; a[6] += lk * lk;
        a[7] += li * lj; a[8] += li * lk; a[9] += lj * lk;
        a[10] = li < a[10] ? li : a[10]; a[11] = lj < a[11] ? lj : a[11]; a[12] = lk < a[12] ? lk : a[12];
        a[13] = li > a[13] ? li : a[13]; a[14] = lj > a[14] ? lj : a[14]; a[15] = lk > a[15] ? lk : a[15];
    }
#pragma unroll
    for (int c = 0; c < 10; ++c) a[c] = wave_sum(a[c]);
#pragma unroll
    for (int c = 10; c < 13; ++c) a[c] = wave_min(a[c]);
#pragma unroll
    for (int c = 13; c < 16; ++c) a[c] = wave_max(a[c]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < SMIL_HULL_STATS; ++c) s_red[wave][c] = a[c];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < HULL_THREADS / 64; ++w) {
        for (int c = 0; c < 10; ++c) a[c] += s_red[w][c];
        for (int c = 10; c < 13; ++c) a[c] = s_red[w][c] < a[c] ? s_red[w][c] : a[c];
        for (int c = 13; c < 16; ++c) a[c] = s_red[w][c] > a[c] ? s_red[w][c] : a[c];
    }
    if (a[0] == 0) return;  // (an empty block leaves the preset row as it is)
    long long *s = stats + SMIL_HULL_STATS * (size_t)frame;
    for (int c = 0; c < 10; ++c) atomicAdd((unsigned long long *)(s + c), (unsigned long long)a[c]);
    for (int c = 10; c < 13; ++c) atomicMin(s + c, a[c]);
    for (int c = 13; c < 16; ++c) atomicMax(s + c, a[c]);
}

// ---- surface ----------------------------------------------------------------------------------------------------------------
// occupied, and a 6-neighbour is not (the grid's border counts as unoccupied)
__device__ __forceinline__ bool hull_is_surface(const unsigned char *o, long long v, const HullGridDev &g, bool small) {
    if (!o[v]) return false;
    int i, j, k;
    hull_decode(v, g.Gx, g.Gy, small, i, j, k);
    if (i == 0 || i == g.Gx - 1 || j == 0 || j == g.Gy - 1 || k == 0 || k == g.Gz - 1) return true;
    const long long sy = g.Gx, sz = (long long)g.Gx * g.Gy;
    const unsigned char xm = o[v - 1], xp = o[v + 1], ym = o[v - sy], yp = o[v + sy], zm = o[v - sz], zp = o[v + sz];
    return !(xm && xp && ym && yp && zm && zp);
}

template <bool WRITE>
__global__ void __launch_bounds__(HULL_THREADS) k_hull_surface(const unsigned char *occ, HullGridDev g, long long *counts, float *points,
                                                               long long *index) {
    __shared__ int s_wave[HULL_THREADS / 64];
    const long long frame = (long long)(blockIdx.x / (unsigned long long)g.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)g.chunks);
    const unsigned char *o = occ + (size_t)frame * (size_t)g.vox;
    const bool small = g.vox <= 0x7FFFFFFFLL;
    const long long v0 = (chunk * HULL_THREADS + threadIdx.x) * HULL_SURF_VOX;
    bool flag[HULL_SURF_VOX];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < HULL_SURF_VOX; ++q) {
        flag[q] = v0 + q < g.vox && hull_is_surface(o, v0 + q, g, small);
        mine += flag[q] ? 1 : 0;
    }
    int total;
    const int before = block_scan_exclusive<int, HULL_THREADS>(mine, s_wave, total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
        return;
    }
    long long pos = counts[blockIdx.x] + before;  // (counts: the exclusive prefixes k_hull_scan left)
    const double *org = g.origin + 3 * (frame % g.n_origin);
    const double voxel = g.voxel[frame % g.n_voxel];
#pragma unroll
    for (int q = 0; q < HULL_SURF_VOX; ++q) {
        if (!flag[q]) continue;
        int i, j, k;
        hull_decode(v0 + q, g.Gx, g.Gy, small, i, j, k);
        points[3 * pos] = (float)hull_centre(org[0], i, voxel);
        points[3 * pos + 1] = (float)hull_centre(org[1], j, voxel);
        points[3 * pos + 2] = (float)hull_centre(org[2], k, voxel);
        if (index) index[pos] = v0 + q;
        ++pos;
    }
}

// The scan of hull_grid.h: workgroup blockIdx.x takes job blockIdx.x, HULL_SCAN_THREADS counts a round, the rounds before it in `carry`.
struct HullScanArgs {  // (the sizes first: the kernel reads n before anything else, and with the first job they fill 56 bytes)
    long long n, chunks;
    int N;
    HullScanJob job[2];
};

__global__ void __launch_bounds__(HULL_SCAN_THREADS) k_hull_scan(HullScanArgs a) {
    __shared__ long long s_wave[HULL_SCAN_THREADS / 64];
    const HullScanJob &j = blockIdx.x ? a.job[1] : a.job[0];
    long long carry = 0;
    for (long long base = 0; base < a.n; base += HULL_SCAN_THREADS) {
        const long long e = base + threadIdx.x;
        long long total;
        const long long excl = carry + block_scan_exclusive<long long, HULL_SCAN_THREADS>(e < a.n ? j.counts[e] : 0, s_wave, total);
        __syncthreads();  // (the next round rewrites s_wave)
        if (e < a.n) {
            j.counts[e] = excl;
            if (e % a.chunks == 0) j.offsets[e / a.chunks] = j.scale * excl;
        }
        carry += total;
    }
    if (threadIdx.x != 0) return;
    if (j.write_total_at_n) j.counts[a.n] = carry;
    j.offsets[a.N] = j.scale * carry;
}

int hull_scan(const HullScanJob *jobs, int n_jobs, long long n, long long chunks, int N, hipStream_t stream) {
    const HullScanArgs a{n, chunks, N, {jobs[0], jobs[n_jobs - 1]}};
    hipLaunchKernelGGL(k_hull_scan, dim3((unsigned)n_jobs), dim3(HULL_SCAN_THREADS), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static int check_hull_lookup(const char *who, const void *masks, int H, int W, float threshold, const SmilCameras *cam, int N, HullLookup *out) {
    SMIL_REQUIRE(cam && cam->R && cam->T && cam->fov, "%s: a camera table is missing", who);
    SMIL_REQUIRE(cam->views >= 1 && cam->views <= SMIL_HULL_MAX_VIEWS, "%s: views=%d outside 1..%d", who, cam->views, SMIL_HULL_MAX_VIEWS);
    SMIL_REQUIRE((long long)cam->N == (long long)N * cam->views, "%s: cameras hold N=%d images, expected %d frames x %d views", who, cam->N, N,
                 cam->views);
    SMIL_REQUIRE(cam->S >= 1, "%s: S=%d", who, cam->S);
    const int rows[5] = {cam->nR, cam->nT, cam->nFov, cam->aspect ? cam->nAspect : 1, cam->principal ? cam->nPrincipal : 1};
    const char *names[5] = {"R", "T", "fov", "aspect", "principal"};
    for (int k = 0; k < 5; ++k)
        SMIL_REQUIRE(rows[k] == 1 || rows[k] == cam->views || rows[k] == cam->N, "%s: camera table %s has %d rows; expected 1, views=%d or N*views=%d",
                     who, names[k], rows[k], cam->views, cam->N);
    SMIL_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 0x7FFFFFFFLL, "%s: masks of %d x %d pixels", who, H, W);
    SMIL_REQUIRE(threshold == threshold, "%s: the threshold is NaN", who);
    SMIL_REQUIRE(masks, "%s: null masks", who);
    *out = HullLookup{masks, *cam, H, W, threshold, 0};
    return SMIL_OK;
}

extern "C" size_t smil_hull_carve_workspace_bytes(const SmilHullGrid *g) {
    if (!g || g->n_origin < 1 || g->n_voxel_size < 1) return 0;
    return hull_layout(nullptr, g, 0).bytes;
}

extern "C" int smil_hull_carve(const SmilHullGrid *g, const void *masks, int32_t masks_f32, int32_t H, int32_t W, float threshold,
                               const SmilCameras *cam, int32_t min_views, int32_t max_misses, int32_t outside_carves, uint8_t *occ, uint8_t *fg,
                               uint8_t *seen, void *workspace, void *stream_) {
    long long vox;
    if (int rc = check_hull_grid("smil_hull_carve", g, true, &vox)) return rc;
    CarveArgs a;
    if (int rc = check_hull_lookup("smil_hull_carve", masks, H, W, threshold, cam, g->N, &a.look)) return rc;
    SMIL_REQUIRE(min_views >= 0 && min_views <= cam->views, "smil_hull_carve: min_views=%d outside 0..views=%d", min_views, cam->views);
    SMIL_REQUIRE(max_misses >= 0, "smil_hull_carve: max_misses=%d is negative", max_misses);
    SMIL_REQUIRE(occ && workspace, "smil_hull_carve: null occ or workspace");
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = hull_upload(hull_layout(workspace, g, 0), g, vox, HULL_VOX * HULL_THREADS, &a.g, stream)) return rc;
    a.look.outside_carves = outside_carves != 0;
    a.min_views = min_views; a.max_misses = max_misses;
    a.occ = occ; a.fg = fg; a.seen = seen;
    const dim3 grid((unsigned)(a.g.chunks * g->N));
    if (masks_f32) hipLaunchKernelGGL(k_hull_carve<float>, grid, dim3(HULL_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_hull_carve<unsigned char>, grid, dim3(HULL_THREADS), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_hull_query(const float *points, int32_t N, int64_t P, const void *masks, int32_t masks_f32, int32_t H, int32_t W,
                               float threshold, const SmilCameras *cam, int32_t outside_carves, uint8_t *fg, uint8_t *seen, void *stream_) {
    SMIL_REQUIRE(N >= 1 && P >= 0, "smil_hull_query: bad sizes N=%d P=%lld", N, (long long)P);
    QueryArgs a;
    if (int rc = check_hull_lookup("smil_hull_query", masks, H, W, threshold, cam, N, &a.look)) return rc;
    a.chunks = hull_chunks(P, HULL_THREADS);
    SMIL_REQUIRE(a.chunks <= 0x7FFFFFFFLL / N, "smil_hull_query: N=%d frames of %lld points exceed the grid", N, (long long)P);
    if (P == 0) return SMIL_OK;
    SMIL_REQUIRE(points && fg && seen, "smil_hull_query: null argument");
    a.look.outside_carves = outside_carves != 0;
    a.points = points; a.P = P; a.fg = fg; a.seen = seen;
    const dim3 grid((unsigned)(a.chunks * N));
    if (masks_f32) hipLaunchKernelGGL(k_hull_query<float>, grid, dim3(HULL_THREADS), 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL(k_hull_query<unsigned char>, grid, dim3(HULL_THREADS), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_hull_stats(const SmilHullGrid *g, const uint8_t *occ, int64_t *stats, void *stream_) {
    long long vox;
    if (int rc = check_hull_grid("smil_hull_stats", g, false, &vox)) return rc;
    SMIL_REQUIRE(occ && stats, "smil_hull_stats: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    const HullGridDev d{nullptr, nullptr, 1, 1, g->Gx, g->Gy, g->Gz, vox, hull_chunks(vox, HULL_STAT_VOX * HULL_THREADS)};
    hipLaunchKernelGGL(k_hull_stats_init, dim3((unsigned)((g->N + 255) / 256)), dim3(256), 0, stream, (long long *)stats, g->N, g->Gx, g->Gy, g->Gz);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hull_stats, dim3((unsigned)(d.chunks * g->N)), dim3(HULL_THREADS), 0, stream, (const unsigned char *)occ, d, (long long *)stats);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" size_t smil_hull_surface_workspace_bytes(const SmilHullGrid *g) {
    if (!hull_extent_ok(g) || g->n_origin < 1 || g->n_voxel_size < 1) return 0;
    return hull_layout(nullptr, g, hull_chunks((long long)g->Gx * g->Gy * g->Gz, HULL_SURF_VOX * HULL_THREADS) * g->N).bytes;
}

extern "C" int smil_hull_surface_count(const SmilHullGrid *g, const uint8_t *occ, int64_t *offsets, void *workspace, void *stream_) {
    long long vox;
    if (int rc = check_hull_grid("smil_hull_surface_count", g, false, &vox)) return rc;
    SMIL_REQUIRE(g->n_origin >= 1 && g->n_voxel_size >= 1, "smil_hull_surface_count: the grid's table sizes lay out the workspace: %d, %d", g->n_origin,
                 g->n_voxel_size);
    SMIL_REQUIRE(occ && offsets && workspace, "smil_hull_surface_count: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    const HullGridDev d{nullptr, nullptr, 1, 1, g->Gx, g->Gy, g->Gz, vox, hull_chunks(vox, HULL_SURF_VOX * HULL_THREADS)};
    const HullWorkspace w = hull_layout(workspace, g, d.chunks * g->N);
    hipLaunchKernelGGL(k_hull_surface<false>, dim3((unsigned)(d.chunks * g->N)), dim3(HULL_THREADS), 0, stream, (const unsigned char *)occ, d, w.counts,
                       (float *)nullptr, (long long *)nullptr);
    SMIL_LAUNCH_CHECK();
    const HullScanJob job{w.counts, (long long *)offsets, 1, 0};
    return hull_scan(&job, 1, d.chunks * g->N, d.chunks, g->N, stream);
}

extern "C" int smil_hull_surface_write(const SmilHullGrid *g, const uint8_t *occ, void *workspace, float *points, int64_t *index, void *stream_) {
    long long vox;
    if (int rc = check_hull_grid("smil_hull_surface_write", g, true, &vox)) return rc;
    SMIL_REQUIRE(occ && workspace && points, "smil_hull_surface_write: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    HullGridDev d;
    const HullWorkspace w = hull_layout(workspace, g, hull_chunks(vox, HULL_SURF_VOX * HULL_THREADS) * g->N);
    if (int rc = hull_upload(w, g, vox, HULL_SURF_VOX * HULL_THREADS, &d, stream)) return rc;
    hipLaunchKernelGGL(k_hull_surface<true>, dim3((unsigned)(d.chunks * g->N)), dim3(HULL_THREADS), 0, stream, (const unsigned char *)occ, d, w.counts,
                       points, (long long *)index);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
