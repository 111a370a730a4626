// Multi-view keypoint triangulation for gfx950: DLT over the valid views of every (frame, keypoint) problem, with the reference's
// pair RANSAC in front of it.  Everything is float64, as the reference computes it.
//
// Replaces (reference): smal_fitter/sleap_data/triangulate_3d_points.py triangulate_all (:830-978, a Python loop over frames x
// keypoints x cameras), with triangulate_point_dlt (:156-176), reprojection_errors_vectorized (:179-194), triangulate_point_ransac
// (:205-281) and undistort_points (:284-301) inside it.
//
//  * k_triangulate     one wave per problem, TRI_WAVES problems per workgroup, no barrier, no atomics, nothing shared between problems.
//      load            lane c is camera c: the view filter of :905-927, the undistortion of :922-924 in the lane, a ballot, and the
//                      valid views compacted in camera order into the wave's LDS slice (projection matrix, point, the two DLT rows).
//      hypotheses      lane h is pair h of the table for this n (:240-245; built on the host, the generator is not restated here): the
//                      null vector of its 4 x 4 system by one-sided Jacobi in registers, then the n reprojection errors with the
//                      views' matrices broadcast from LDS (:262-264).  The winner is the wave maximum of {count, 63 - lane}: the
//                      lowest-index hypothesis of the largest count, which is what the strict `>` of :266 keeps.
//      final system    lane r is row r of the 2n x 4 system (<= 64 rows: one wave), rows of views outside the winner's mask zero (they
//                      change no singular vector).  Four Householder reflections with ten wave sums leave R in lanes 0 .. 3; every lane
//                      then runs the same 4 x 4 Jacobi on R, so the hypotheses and the final system share one solver.  A serial walk
//                      of one lane over the 64 rows would leave 63 lanes idle for ~250 dependent rotations.
//      errors          lane c again: the reprojection error of the final point in camera c (:951), their mean over the n valid views.
//    The Jacobi works on A, not on A^T A: the smallest singular vector of a DLT system is decided at the rounding level of A, and the
//    normal equations square its condition number.
#include <cmath>

#include "common.h"

#define TRI_WAVES 4    // problems of one workgroup
#define TRI_SWEEPS 12  // cap of the Jacobi sweeps (a 4 x 4 system is through after 5 - 7; NaN input rotates until the cap and stays NaN)

struct TriArgs {
    const double *P;       // (C, 3, 4)
    const double *K;       // (C, 3, 3) or null
    const double *dist;    // (C, 5) or null
    const double *obs;     // (NP, C, 2)
    const double *scores;  // (NP, C) or null
    const int *pairs;      // (SMIL_TRI_MAX_VIEWS + 1, SMIL_TRI_MAX_HYP, 2), row n: the hypotheses of n views
    long long NP;
    int C, min_views, mode;
    double conf, thr;
    double *xyz, *mean_err, *view_err, *undist;
    int *status, *views_used;
    unsigned int *inlier_mask;
};

// One view of a problem in LDS: its projection matrix, its (undistorted) point and its two DLT rows x P[2] - P[0], y P[2] - P[1].
struct TriView {
    double P[12], pt[2], row[2][4];
};

// The right singular vector of the smallest singular value of the 4 x 4 matrix a (rows a[i]), by one-sided (Hestenes) Jacobi:
// columns p, q are rotated until every pair is orthogonal, V collects the rotations, and the column of the smallest norm names the
// vector.  The loop leaves when no lane of the wave has rotated in a sweep (wave-uniform: the lanes are hypotheses).
__device__ __forceinline__ void null_vector4(double (&a)[4][4], double (&x)[4]) {
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TRI_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    al += a[k][p] * a[k][p];
                    be += a[k][q] * a[k][q];
                    ga += a[k][p] * a[k][q];
                }
                // (written so that a NaN rotates: it spreads to the result instead of stopping the sweeps on a finite guess)
                const bool rot = !(fabs(ga) <= 0x1p-52 * sqrt(al * be));
                rotated |= rot;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = rot ? 1.0 / sqrt(1.0 + t * t) : 1.0, s = rot ? c * t : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ap = a[k][p], aq = a[k][q], vp = v[k][p], vq = v[k][q];
                    a[k][p] = rot ? c * ap - s * aq : ap;
                    a[k][q] = rot ? s * ap + c * aq : aq;
                    v[k][p] = rot ? c * vp - s * vq : vp;
                    v[k][q] = rot ? s * vp + c * vq : vq;
                }
            }
        }
        if (!__any(rotated)) break;
    }
    double best = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double nj = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) nj += a[k][j] * a[k][j];
        const bool take = j == 0 || nj < best || nj != nj;
        best = take ? nj : best;
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = take ? v[k][j] : x[k];
    }
}

// ||proj_xy / proj_z - pt|| of the point X in one view (:191-194)
__device__ __forceinline__ double reproj_error(const TriView &w, double X0, double X1, double X2) {
    const double px = ((w.P[0] * X0 + w.P[1] * X1) + w.P[2] * X2) + w.P[3];
    const double py = ((w.P[4] * X0 + w.P[5] * X1) + w.P[6] * X2) + w.P[7];
    const double pz = ((w.P[8] * X0 + w.P[9] * X1) + w.P[10] * X2) + w.P[11];
    const double dx = px / pz - w.pt[0], dy = py / pz - w.pt[1];
    return sqrt(dx * dx + dy * dy);
}

// cv2.undistortPoints(pts, K, dist, P=K) as documented: normalise by fx, fy, cx, cy, five rounds of the fixed-point iteration
// x <- (x0 - tangential(x)) / radial(x), back through K (:284-301)
__device__ __forceinline__ void undistort5(const double *K, const double *d, double &u, double &v) {
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    const double x0 = (u - K[2]) / K[0], y0 = (v - K[5]) / K[4];
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    const double w = K[6] * x + K[7] * y + K[8];
    u = (K[0] * x + K[1] * y + K[2]) / w;
    v = (K[3] * x + K[4] * y + K[5]) / w;
}

__global__ void __launch_bounds__(64 * TRI_WAVES) k_triangulate(TriArgs a) {
    __shared__ TriView s_view[TRI_WAVES][SMIL_TRI_MAX_VIEWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long prob = (long long)blockIdx.x * TRI_WAVES + wave;
    if (prob >= a.NP) return;  // (wave-uniform; the kernel has no barrier)
    TriView *views = s_view[wave];
    const int C = a.C;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);

    // ---- load: lane c is camera c ----
    bool valid = false;
    double u = 0.0, v = 0.0;
    if (lane < C) {
        const size_t o = (size_t)prob * C + lane;
        u = a.obs[2 * o];
        v = a.obs[2 * o + 1];
        valid = true;
        if (!(a.mode & SMIL_TRI_KEEP_ALL_VIEWS)) {
            const double sc = a.scores ? a.scores[o] : nan;
            valid = !(u != u || v != v) && !(sc == sc && sc < a.conf) && !(u == 0.0 && v == 0.0);
        }
    }
    const unsigned long long vmask = __ballot(valid);
    const int n = __popcll(vmask);
    const int ci = __popcll(vmask & ((1ull << lane) - 1ull));  // the view's place among the valid ones
    if (valid) {
        if (a.K && a.dist) {
            const double *d = a.dist + 5 * lane;
            bool zero = true;  // np.allclose(dist, 0): every |d| <= 1e-8 (a NaN coefficient is not close)
            for (int i = 0; i < 5; ++i) zero &= fabs(d[i]) <= 1e-8;
            if (!zero) undistort5(a.K + 9 * lane, d, u, v);
        }
        if (a.undist) {
            a.undist[2 * ((size_t)prob * C + lane)] = u;
            a.undist[2 * ((size_t)prob * C + lane) + 1] = v;
        }
        TriView &w = views[ci];
        const double *P = a.P + 12 * lane;
#pragma unroll
        for (int i = 0; i < 12; ++i) w.P[i] = P[i];
        w.pt[0] = u;
        w.pt[1] = v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w.row[0][j] = u * P[8 + j] - P[j];
            w.row[1][j] = v * P[8 + j] - P[4 + j];
        }
    }
    // (the slice is this wave's own and a wave runs in lockstep: the LDS writes above are ordered before the reads below)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    int status = 0, used = n;
    unsigned int cmask = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);  // views of the final system, compacted numbering
    if (n < a.min_views) {
        status = 1;
    } else if ((a.mode & SMIL_TRI_RANSAC) && n >= 3) {
        // ---- hypotheses: lane h is pair h ----
        const int H = min(n * (n - 1) / 2, SMIL_TRI_MAX_HYP);
        int key = -1;
        unsigned int hmask = 0;
        if (lane < H) {
            const int *pr = a.pairs + ((size_t)n * SMIL_TRI_MAX_HYP + lane) * 2;
            const int i = min(max(pr[0], 0), n - 1), j = min(max(pr[1], 0), n - 1);
            double A[4][4], X[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                A[0][c] = views[i].row[0][c];
                A[1][c] = views[i].row[1][c];
                A[2][c] = views[j].row[0][c];
                A[3][c] = views[j].row[1][c];
            }
            null_vector4(A, X);
            const double X0 = X[0] / X[3], X1 = X[1] / X[3], X2 = X[2] / X[3];
            for (int k = 0; k < n; ++k)
                if (reproj_error(views[k], X0, X1, X2) < a.thr) hmask |= 1u << k;  // strict; a NaN error is no inlier
            key = (__popc(hmask) << 6) | (63 - lane);
        }
        const int best = __builtin_amdgcn_readfirstlane(wave_max(key));
        used = best >> 6;
        if (used < a.min_views) status = 2;
        else cmask = (unsigned int)read_lane((int)hmask, 63 - (best & 63));
    }

    double X0 = nan, X1 = nan, X2 = nan;
    if (status == 0) {
        // ---- the final 2n x 4 system: lane r is row r ----
        double r[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < 2 * n && ((cmask >> (lane >> 1)) & 1u)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = views[lane >> 1].row[lane & 1][j];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // Householder reflection k: column k becomes (.., alpha, 0, ..)
            const double x = lane >= k ? r[k] : 0.0;
            const double sigma = wave_sum(x * x), norm = sqrt(sigma);
            const double akk = read_lane(r[k], k);
            const double alpha = akk >= 0.0 ? -norm : norm;
            const double h = lane == k ? akk - alpha : x;       // the reflector
            const double hth = 2.0 * norm * (norm + fabs(akk));  // its squared length
#pragma unroll
            for (int j = k + 1; j < 4; ++j) {
                const double s = wave_sum(h * r[j]);
                const double f = hth != 0.0 ? 2.0 * s / hth : 0.0;  // (a zero column stays)
                r[j] -= f * h;
            }
            r[k] = lane == k ? alpha : (lane > k ? 0.0 : r[k]);
        }
        double R[4][4], X[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) R[i][j] = j >= i ? read_lane(r[j], i) : 0.0;
        null_vector4(R, X);
        X0 = X[0] / X[3];
        X1 = X[1] / X[3];
        X2 = X[2] / X[3];
    }

    // ---- errors: lane c is camera c again ----
    const double err = (status == 0 && valid) ? reproj_error(views[ci], X0, X1, X2) : nan;
    const double mean = status == 0 ? wave_sum(valid ? err : 0.0) / (double)n : nan;
    if (a.view_err && lane < C) a.view_err[(size_t)prob * C + lane] = err;
    const unsigned long long in = __ballot(status == 0 && valid && ((cmask >> ci) & 1u));
    if (lane == 0) {
        a.xyz[3 * prob] = X0;
        a.xyz[3 * prob + 1] = X1;
        a.xyz[3 * prob + 2] = X2;
        a.status[prob] = status;
        a.views_used[prob] = status == 0 ? used : 0;
        a.mean_err[prob] = mean;
        if (a.inlier_mask) a.inlier_mask[prob] = (unsigned int)in;
    }
}

extern "C" int smil_triangulate(const double *P, const double *K, const double *dist, const double *obs, const double *scores,
                                const int32_t *pairs, int64_t N, int32_t Kp, int32_t C, double confidence_threshold, int32_t min_views,
                                double reproj_threshold, int32_t mode, double *xyz, int32_t *status, int32_t *views_used, double *mean_err,
                                double *view_err, uint32_t *inlier_mask, double *obs_undistorted, void *stream_) {
    SMIL_REQUIRE(N > 0 && Kp > 0 && C > 0, "smil_triangulate: bad sizes N=%lld Kp=%d C=%d", (long long)N, Kp, C);
    if (const int rc = smil_check_views("smil_triangulate", C, "a problem's rows stay in one wave")) return rc;
    if (const int rc = smil_check_grid("smil_triangulate", N, Kp, TRI_WAVES)) return rc;
    SMIL_REQUIRE(min_views >= 1, "smil_triangulate: min_views=%d must be >= 1", min_views);
    SMIL_REQUIRE((mode & ~(SMIL_TRI_RANSAC | SMIL_TRI_KEEP_ALL_VIEWS)) == 0, "smil_triangulate: unknown mode bits %d", mode);
    SMIL_REQUIRE(P && obs && xyz && status && views_used && mean_err, "smil_triangulate: null argument");
    SMIL_REQUIRE((K == nullptr) == (dist == nullptr), "smil_triangulate: K and dist come together");
    SMIL_REQUIRE(pairs || !(mode & SMIL_TRI_RANSAC), "smil_triangulate: RANSAC needs the pair table");
    TriArgs a;
    a.P = P; a.K = K; a.dist = dist; a.obs = obs; a.scores = scores; a.pairs = (const int *)pairs;
    a.NP = (long long)N * Kp; a.C = C; a.min_views = min_views; a.mode = mode;
    a.conf = confidence_threshold; a.thr = reproj_threshold;
    a.xyz = xyz; a.mean_err = mean_err; a.view_err = view_err; a.undist = obs_undistorted;
    a.status = (int *)status; a.views_used = (int *)views_used; a.inlier_mask = inlier_mask;
    const unsigned blocks = (unsigned)((a.NP + TRI_WAVES - 1) / TRI_WAVES);
    hipLaunchKernelGGL(k_triangulate, dim3(blocks), dim3(64 * TRI_WAVES), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
