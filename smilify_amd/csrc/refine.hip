// Multi-view camera refinement for gfx950: every camera's 6 or 10 parameters (rvec, t, fx, fy, cx, cy) fitted to its 3-D / 2-D
// correspondences by a robust Levenberg-Marquardt, all cameras at once.  Everything is float64, as the reference computes it.
//
// Replaces (reference): smal_fitter/sleap_data/refine_camera_params.py optimize_camera (:171-226: scipy least_squares, method "trf",
// loss "soft_l1", a numerical Jacobian of 11 residual evaluations, one camera after the other) with reprojection_residuals (:143-163).
//
//  * k_refine_accumulate   grid (blocks, cameras), REF_THREADS lanes.  Every lane walks its camera's correspondences at the stride of
//      the grid and keeps the cost, g = J^T (w f) and the upper triangle of H = J^T diag(w) J of its points in registers (1 + 10 + 55
//      values for 10 parameters, 1 + 6 + 21 for 6); the waves reduce with wave_sum, the workgroup's waves are added in wave order
//      through LDS, and the block writes ONE partial of REF_SLOTS doubles.  No atomics: the order of every sum follows from the count
//      and the launch shape alone.  The parameters are the camera's CANDIDATE; a camera that is done returns at once.
//      The rotation is never formed: with p = r x X and q = r x p, R X = X + a p + b q (a = sin(th) / th, b = (1 - cos(th)) / th^2),
//      and d(R X)/d r_k = r_k (a1 p + b1 q) + a e_k x X + b (e_k x p + r x (e_k x X)) with a1 = (cos(th) - a) / th^2 and
//      b1 = (a - 2 b) / th^2; below th^2 = 1e-3 the four coefficients come from their series, so r = 0 gives R = I and the
//      generators.  That keeps five coefficients and r in registers instead of four 3 x 3 matrices.
//  * k_refine_step         one wave per camera.  The lanes add the partials in block order; lane 0 then applies lm.h's rules (shared
//      with refine_points.hip: soft_l1, accept / reject, the Cholesky solve with L and delta in LDS, the statuses) for the next candidate.
//  * smil_refine_cameras   enqueues at most max_steps (accumulate, step) pairs and reads the done flags every REF_POLL pairs.
//      There is no device-side loop whose trip count depends on the data and no host read inside a pair.
#include <cmath>

#include "common.h"
#include "lm.h"

#define REF_THREADS 256    // lanes of an accumulation workgroup: "one block's worth" of correspondences
#define REF_MAX_BLOCKS 64  // workgroups per camera at most (200 000 correspondences: 13 per lane)
#define REF_SLOTS 66       // doubles of one partial: cost, g (10), upper triangle of H (55); 6 parameters use the first 28
#define REF_POLL 8         // (accumulate, step) pairs between two reads of the done flags
#define REF_FRESH 0        // phase of a camera: no evaluation yet / iterating / done
#define REF_RUN 1
#define REF_DONE 2

struct RefineArgs {
    const double *pts3, *pts2;  // (sum M, 3), (sum M, 2)
    const long long *offsets;   // (C + 1)
    const double *eval_params;  // (C, 10): evaluate here and ignore the phases (smil_refine_evaluate), or null
    double f_scale;
    int n_blocks, np;
    // state of the iteration; the outputs of smil_refine_cameras are part of it
    double *cur, *cand, *g, *H, *cost, *cost0, *lambda;  // (C,10) (C,10) (C,10) (C,55) (C) (C) (C)
    int *phase, *status, *n_accept, *n_trial;
    double *partials;  // (C, n_blocks, REF_SLOTS)
};

// sin(th)/th, (1 - cos(th))/th^2 and the coefficients of their derivatives along r, from th^2
__device__ __forceinline__ void rodrigues_coefficients(double t2, double &a, double &b, double &a1, double &b1) {
    if (t2 < 1e-3) {  // the next terms are below t2^4 / 9! < 3e-18 of the first
        a = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0)));
        b = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0)));
        a1 = -1.0 / 3.0 + t2 * (1.0 / 30.0 + t2 * (-1.0 / 840.0 + t2 * (1.0 / 45360.0)));
        b1 = -1.0 / 12.0 + t2 * (1.0 / 180.0 + t2 * (-1.0 / 6720.0 + t2 * (1.0 / 453600.0)));
    } else {
        const double th = sqrt(t2), s = sin(th), c = cos(th);
        a = s / th;
        b = (1.0 - c) / t2;
        a1 = (c - a) / t2;
        b1 = (a - 2.0 * b) / t2;
    }
}

template <int NP>
__global__ void __launch_bounds__(REF_THREADS) k_refine_accumulate(RefineArgs A) {
    constexpr int NACC = 1 + NP + NP * (NP + 1) / 2;
    __shared__ double s_part[REF_THREADS / 64][NACC];
    const int cam = blockIdx.y;
    if (!A.eval_params && A.phase[cam] == REF_DONE) return;  // (block-uniform, in front of the barrier)
    const double *prm = (A.eval_params ? A.eval_params : A.cand) + 10 * (size_t)cam;
    const double r0 = prm[0], r1 = prm[1], r2 = prm[2], t0 = prm[3], t1 = prm[4], t2_ = prm[5];
    const double fx = prm[6], fy = prm[7], cx = prm[8], cy = prm[9];
    double a, b, a1, b1;
    rodrigues_coefficients((r0 * r0 + r1 * r1) + r2 * r2, a, b, a1, b1);
    const double inv_fs = 1.0 / A.f_scale;

    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

    const long long first = A.offsets[cam], M = A.offsets[cam + 1] - first;
    const long long stride = (long long)A.n_blocks * REF_THREADS;
    for (long long i = (long long)blockIdx.x * REF_THREADS + threadIdx.x; i < M; i += stride) {
        const double *X = A.pts3 + 3 * (first + i), *o = A.pts2 + 2 * (first + i);
        const double X0 = X[0], X1 = X[1], X2 = X[2];
        const double p0 = r1 * X2 - r2 * X1, p1 = r2 * X0 - r0 * X2, p2 = r0 * X1 - r1 * X0;  // r x X
        const double q0 = r1 * p2 - r2 * p1, q1 = r2 * p0 - r0 * p2, q2 = r0 * p1 - r1 * p0;  // r x (r x X)
        const double x = ((X0 + a * p0) + b * q0) + t0, y = ((X1 + a * p1) + b * q1) + t1, z = ((X2 + a * p2) + b * q2) + t2_;
        const double iz = 1.0 / z, xn = x * iz, yn = y * iz;  // (z <= 0 divides as IEEE does)
        const double fu = (fx * xn + cx) - o[0], fv = (fy * yn + cy) - o[1];
        double rho_u, rho_v, wu, wv;  // soft_l1 of every scalar residual
        soft_l1(fu * inv_fs, rho_u, wu);
        soft_l1(fv * inv_fs, rho_v, wv);
        acc[0] += rho_u + rho_v;

        // rows of the Jacobian: d(u, v) / d(x, y, z) through d(x, y, z) / d(r, t), then the intrinsics
        const double ux = fx * iz, uz = -fx * xn * iz, vy = fy * iz, vz = -fy * yn * iz;
        const double m0 = a1 * p0 + b1 * q0, m1 = a1 * p1 + b1 * q1, m2 = a1 * p2 + b1 * q2;
        double Ju[NP], Jv[NP];
        {
            // e_0 x X = (0, -X2, X1); e_0 x p = (0, -p2, p1); r x (e_0 x X) = (r1 X1 + r2 X2, -r0 X1, -r0 X2)
            const double d0 = r0 * m0 + b * (r1 * X1 + r2 * X2);
            const double d1 = r0 * m1 - a * X2 + b * (-p2 - r0 * X1);
            const double d2 = r0 * m2 + a * X1 + b * (p1 - r0 * X2);
            Ju[0] = ux * d0 + uz * d2;
            Jv[0] = vy * d1 + vz * d2;
        }
        {
            // e_1 x X = (X2, 0, -X0); e_1 x p = (p2, 0, -p0); r x (e_1 x X) = (-r1 X0, r0 X0 + r2 X2, -r1 X2)
            const double d0 = r1 * m0 + a * X2 + b * (p2 - r1 * X0);
            const double d1 = r1 * m1 + b * (r0 * X0 + r2 * X2);
            const double d2 = r1 * m2 - a * X0 + b * (-p0 - r1 * X2);
            Ju[1] = ux * d0 + uz * d2;
            Jv[1] = vy * d1 + vz * d2;
        }
        {
            // e_2 x X = (-X1, X0, 0); e_2 x p = (-p1, p0, 0); r x (e_2 x X) = (-r2 X0, -r2 X1, r0 X0 + r1 X1)
            const double d0 = r2 * m0 - a * X1 + b * (-p1 - r2 * X0);
            const double d1 = r2 * m1 + a * X0 + b * (p0 - r2 * X1);
            const double d2 = r2 * m2 + b * (r0 * X0 + r1 * X1);
            Ju[2] = ux * d0 + uz * d2;
            Jv[2] = vy * d1 + vz * d2;
        }
        Ju[3] = ux; Ju[4] = 0.0; Ju[5] = uz;
        Jv[3] = 0.0; Jv[4] = vy; Jv[5] = vz;
        if constexpr (NP == 10) {
            Ju[6] = xn; Ju[7] = 0.0; Ju[8] = 1.0; Ju[9] = 0.0;
            Jv[6] = 0.0; Jv[7] = yn; Jv[8] = 0.0; Jv[9] = 1.0;
        }
        const double gu = wu * fu, gv = wv * fv;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            acc[1 + i] += Ju[i] * gu + Jv[i] * gv;
            const double wi = wu * Ju[i], vi = wv * Jv[i];
#pragma unroll
            for (int j = i; j < NP; ++j) acc[1 + NP + i * NP - i * (i - 1) / 2 + (j - i)] += wi * Ju[j] + vi * Jv[j];
        }
    }

#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = wave_sum(acc[i]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) s_part[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < REF_THREADS / 64; ++w) s += s_part[w][threadIdx.x];
        A.partials[((size_t)cam * A.n_blocks + blockIdx.x) * REF_SLOTS + threadIdx.x] = s;
    }
}

// The partials of camera `cam` added in block order into s[0 .. nacc): slot t by lane t (and t + 64).
__device__ __forceinline__ void sum_partials(const RefineArgs &A, int cam, int nacc, double *s) {
    for (int t = threadIdx.x; t < nacc; t += 64) {
        const double *p = A.partials + (size_t)cam * A.n_blocks * REF_SLOTS + t;
        double v = 0.0;
        for (int blk = 0; blk < A.n_blocks; ++blk) v += p[(size_t)blk * REF_SLOTS];
        s[t] = v;
    }
    __syncthreads();
}

// smil_refine_evaluate: cost (C), g (C,10) and the symmetric H (C,10,10) of eval_params, zero outside the n_params block.
__global__ void __launch_bounds__(64) k_refine_collect(RefineArgs A, double *cost, double *g, double *H) {
    __shared__ double s[REF_SLOTS];
    const int cam = blockIdx.x, np = A.np;
    sum_partials(A, cam, 1 + np + np * (np + 1) / 2, s);
    for (int e = threadIdx.x; e < 100; e += 64) {
        const int i = min(e / 10, e % 10), j = max(e / 10, e % 10);
        H[100 * (size_t)cam + e] = j < np ? s[1 + np + i * np - i * (i - 1) / 2 + (j - i)] : 0.0;
    }
    if (threadIdx.x < 10) g[10 * (size_t)cam + threadIdx.x] = (int)threadIdx.x < np ? s[1 + threadIdx.x] : 0.0;
    if (threadIdx.x == 0) cost[cam] = 0.5 * A.f_scale * A.f_scale * s[0];
}

__global__ void __launch_bounds__(64) k_refine_init(RefineArgs A, const double *params0, int C) {
    const int cam = blockIdx.x * 64 + threadIdx.x;
    if (cam >= C) return;
    const bool skipped = A.offsets[cam + 1] - A.offsets[cam] < SMIL_REFINE_MIN_POINTS;
    for (int i = 0; i < 10; ++i) {
        A.cur[10 * (size_t)cam + i] = A.cand[10 * (size_t)cam + i] = params0[10 * (size_t)cam + i];
        A.g[10 * (size_t)cam + i] = 0.0;
    }
    A.cost[cam] = A.cost0[cam] = __longlong_as_double(0x7FF8000000000000ll);
    A.lambda[cam] = LM_LAMBDA0;
    A.phase[cam] = skipped ? REF_DONE : REF_FRESH;
    A.status[cam] = skipped ? SMIL_REFINE_SKIPPED : lm_status(0);  // (the step limit, until the camera says otherwise)
    A.n_accept[cam] = A.n_trial[cam] = 0;
}

__global__ void __launch_bounds__(64) k_refine_step(RefineArgs A) {
    __shared__ double s[REF_SLOTS], L[10 * 10], d[10];
    const int cam = blockIdx.x, np = A.np, nh = np * (np + 1) / 2;
    if (A.phase[cam] == REF_DONE) return;  // (block-uniform)
    sum_partials(A, cam, 1 + np + nh, s);
    if (threadIdx.x != 0) return;
    double *cur = A.cur + 10 * (size_t)cam, *cand = A.cand + 10 * (size_t)cam, *g = A.g + 10 * (size_t)cam, *H = A.H + 55 * (size_t)cam;
    LmState st = {A.lambda[cam], A.cost[cam], A.cost0[cam], A.n_accept[cam], A.n_trial[cam], A.phase[cam] == REF_FRESH};
    int r = lm_judge(st, 0.5 * A.f_scale * A.f_scale * s[0]);
    if (r & LM_TAKE) {
        for (int i = 0; i < np; ++i) {
            cur[i] = cand[i];
            g[i] = s[1 + i];
        }
        for (int i = 0; i < nh; ++i) H[i] = s[1 + np + i];
    }
    if (!(r & LM_DONE)) r |= np == 10 ? lm_propose<10>(st, H, g, cur, cand, L, d) : lm_propose<6>(st, H, g, cur, cand, L, d);
    A.lambda[cam] = st.lambda;
    A.cost[cam] = st.cost_cur;
    A.cost0[cam] = st.cost0;
    A.n_accept[cam] = st.n_accept;
    A.n_trial[cam] = st.n_trial;
    A.phase[cam] = r & LM_DONE ? REF_DONE : REF_RUN;
    if (r & LM_DONE) A.status[cam] = lm_status(r);
}

// ---- host ----
struct RefineLayout {
    double *cand, *H, *lambda, *partials;
    int *phase;
    size_t bytes;
};

static int refine_blocks(int64_t max_count) {
    const int64_t b = (max_count + REF_THREADS - 1) / REF_THREADS;
    return (int)(b < 1 ? 1 : (b > REF_MAX_BLOCKS ? REF_MAX_BLOCKS : b));
}

static RefineLayout refine_layout(void *base, int C, int n_blocks) {
    Workspace ws{(char *)base};
    RefineLayout l;
    l.cand = ws.take<double>((size_t)C * 10);
    l.H = ws.take<double>((size_t)C * 55);
    l.lambda = ws.take<double>(C);
    l.phase = ws.take<int>(C);
    l.partials = ws.take<double>((size_t)C * n_blocks * REF_SLOTS);
    l.bytes = ws.used;
    return l;
}

extern "C" size_t smil_refine_workspace_bytes(int32_t C, int64_t max_count) {
    if (C < 1 || max_count < 0) return 0;
    return refine_layout(nullptr, C, refine_blocks(max_count)).bytes;
}

// What both entry points check, in this order, before a device is touched.  offsets is a HOST array.
static int refine_check(const char *who, const double *pts3, const double *pts2, const int64_t *offsets, int32_t C, int32_t n_params,
                        double f_scale, const void *workspace, int64_t *max_count) {
    SMIL_REQUIRE(C > 0, "%s: bad size C=%d", who, C);
    SMIL_REQUIRE(C <= 65535, "%s: C=%d cameras exceed the grid", who, C);
    SMIL_REQUIRE(n_params == 6 || n_params == 10, "%s: n_params=%d must be 6 or 10", who, n_params);
    if (const int rc = smil_check_f_scale(who, f_scale)) return rc;
    SMIL_REQUIRE(offsets && workspace, "%s: null argument", who);
    SMIL_REQUIRE(offsets[0] == 0, "%s: offsets[0]=%lld must be 0", who, (long long)offsets[0]);
    int64_t mx = 0;
    for (int c = 0; c < C; ++c) {
        SMIL_REQUIRE(offsets[c + 1] >= offsets[c], "%s: offsets not monotone at camera %d (%lld after %lld)", who, c,
                     (long long)offsets[c + 1], (long long)offsets[c]);
        mx = offsets[c + 1] - offsets[c] > mx ? offsets[c + 1] - offsets[c] : mx;
    }
    SMIL_REQUIRE((pts3 && pts2) || offsets[C] == 0, "%s: null argument", who);
    *max_count = mx;
    return SMIL_OK;
}

static void refine_accumulate(const RefineArgs &a, int C, hipStream_t stream) {
    if (a.np == 10) hipLaunchKernelGGL(k_refine_accumulate<10>, dim3(a.n_blocks, C), dim3(REF_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_refine_accumulate<6>, dim3(a.n_blocks, C), dim3(REF_THREADS), 0, stream, a);
}

extern "C" int smil_refine_evaluate(const double *pts_3d, const double *pts_2d, const int64_t *offsets_host, const int64_t *offsets_dev,
                                    int32_t C, const double *params, int32_t n_params, double f_scale, double *cost, double *g, double *H,
                                    void *workspace, void *stream_) {
    int64_t max_count = 0;
    const int rc = refine_check("smil_refine_evaluate", pts_3d, pts_2d, offsets_host, C, n_params, f_scale, workspace, &max_count);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(offsets_dev && params && cost && g && H, "smil_refine_evaluate: null argument");
    RefineArgs a = {};
    a.n_blocks = refine_blocks(max_count);
    const RefineLayout l = refine_layout(workspace, C, a.n_blocks);
    a.pts3 = pts_3d; a.pts2 = pts_2d; a.offsets = (const long long *)offsets_dev; a.eval_params = params;
    a.f_scale = f_scale; a.np = n_params; a.partials = l.partials;
    hipStream_t stream = (hipStream_t)stream_;
    refine_accumulate(a, C, stream);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_refine_collect, dim3(C), dim3(64), 0, stream, a, cost, g, H);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_refine_cameras(const double *pts_3d, const double *pts_2d, const int64_t *offsets_host, const int64_t *offsets_dev,
                                   int32_t C, const double *params0, int32_t n_params, double f_scale, int32_t max_steps, double *params,
                                   int32_t *status, int32_t *n_accepted, int32_t *n_trials, double *cost0, double *cost, double *g,
                                   void *workspace, void *stream_) {
    int64_t max_count = 0;
    const int rc = refine_check("smil_refine_cameras", pts_3d, pts_2d, offsets_host, C, n_params, f_scale, workspace, &max_count);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(max_steps >= 1, "smil_refine_cameras: max_steps=%d must be >= 1", max_steps);
    SMIL_REQUIRE(offsets_dev && params0 && params && status && n_accepted && n_trials && cost0 && cost && g,
                 "smil_refine_cameras: null argument");
    RefineArgs a = {};
    a.n_blocks = refine_blocks(max_count);
    const RefineLayout l = refine_layout(workspace, C, a.n_blocks);
    a.pts3 = pts_3d; a.pts2 = pts_2d; a.offsets = (const long long *)offsets_dev; a.eval_params = nullptr;
    a.f_scale = f_scale; a.np = n_params;
    a.cur = params; a.cand = l.cand; a.g = g; a.H = l.H; a.cost = cost; a.cost0 = cost0; a.lambda = l.lambda;
    a.phase = l.phase; a.status = (int *)status; a.n_accept = (int *)n_accepted; a.n_trial = (int *)n_trials; a.partials = l.partials;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_refine_init, dim3(ceil_div(C, 64)), dim3(64), 0, stream, a, params0, (int)C);
    SMIL_LAUNCH_CHECK();
    std::vector<int> phase(C);
    for (int step = 0; step < max_steps; ++step) {
        refine_accumulate(a, C, stream);
        SMIL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_refine_step, dim3(C), dim3(64), 0, stream, a);
        SMIL_LAUNCH_CHECK();
        if ((step + 1) % REF_POLL == 0 && step + 1 < max_steps) {
            SMIL_HIP(hipMemcpyAsync(phase.data(), l.phase, sizeof(int) * C, hipMemcpyDeviceToHost, stream));
            SMIL_HIP(hipStreamSynchronize(stream));
            bool all = true;
            for (int c = 0; c < C; ++c) all &= phase[c] == REF_DONE;
            if (all) break;
        }
    }
    return SMIL_OK;
}
