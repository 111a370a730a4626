// Robust nonlinear refinement of triangulated points for gfx950: every (frame, keypoint) point is moved from its start (the DLT point
// of csrc/triangulate.hip) to the minimum of the soft_l1 reprojection cost over its views by a Levenberg-Marquardt in three unknowns,
// all points at once.  Everything is float64.
//
// AN EXTENSION: the reference has no such function (its points stay the DLT points of triangulate_point_dlt).  The soft_l1 cost and
// weight, the accept / reject rule, the Cholesky solve and the statuses are lm.h's, the same code the camera refinement
// (csrc/refine.hip) runs, so the two compose into a block-coordinate bundle adjustment (smilify_amd/refine_points.py).
//
//  * k_refine_points           one wave per problem, RPT_WAVES problems per workgroup, no barrier, no LDS, no atomics, nothing shared
//      between problems.  Lane r is scalar residual r of the at most 2 C = 64: view r >> 1, component r & 1.  It keeps rows
//      r & 1 and 2 of its view's projection matrix and its observed coordinate in registers.  One evaluation is the lane's residual and
//      Jacobian row, then ten wave sums (cost, 3 of g, 6 of H); lanes of views outside the mask contribute exact zeros by SELECTION,
//      so an unwritten, NaN or garbage observation of a dropped view never reaches a sum.  Every lane then runs lm.h's rules and its
//      solve at N = 3, unrolled, in registers: after the butterfly sums all lanes hold the same bits, so the exit of the
//      loop is wave-uniform (and is made a scalar branch with readfirstlane).  Unlike the camera refinement the LM loop runs INSIDE
//      the kernel, bounded by max_steps: the problems are independent and there are millions of them, a host loop of launches would
//      cost a launch pair per step for no shared work (triangulate.hip's Jacobi sweeps are the precedent).
//  * k_refine_points_evaluate  the same accumulation once at given points: cost, g and the symmetric H.
#include <cmath>

#include "common.h"
#include "lm.h"

#define RPT_WAVES 4  // problems of one workgroup

struct RefinePointsArgs {
    const double *P;           // (C, 3, 4)
    const double *obs;         // (NP, C, 2)
    const unsigned int *mask;  // (NP)
    const double *xyz0;        // (NP, 3)
    long long NP;
    int C, max_steps;
    double f_scale;
    double *xyz, *cost0, *cost, *view_err;  // (NP,3) (NP) (NP) (NP,C) or null
    int *status, *n_accept, *n_trial;
    double *g, *H;  // k_refine_points_evaluate: (NP,3) (NP,3,3)
};

// What a lane keeps of its scalar residual: rows k = lane & 1 and 2 of its view's projection matrix and the observed coordinate.
struct RptLane {
    double pk[4], p2[4], o;
    bool active;
};

__device__ __forceinline__ RptLane rpt_load(const RefinePointsArgs &a, long long prob, int lane) {
    RptLane L;
    const int view = lane >> 1, k = lane & 1;
    const unsigned int m = a.mask[prob];
    L.active = view < a.C && ((m >> view) & 1u);
    L.o = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) L.pk[j] = L.p2[j] = 0.0;
    if (L.active) {  // (a dropped view's observation is never read)
        const double *P = a.P + 12 * view;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L.pk[j] = P[4 * k + j];
            L.p2[j] = P[8 + j];
        }
        L.o = a.obs[((size_t)prob * a.C + view) * 2 + k];
    }
    return L;
}

__device__ __forceinline__ int rpt_views(const RefinePointsArgs &a, long long prob) {
    const unsigned int m = a.mask[prob];
    return __popc(a.C >= 32 ? m : (m & ((1u << a.C) - 1u)));
}

// The lane's residual f = h_k / h2 - o at X (h2 <= 0 divides as IEEE does) and, with J, its Jacobian row (P[k,:3] - (h_k / h2) P[2,:3]) / h2.
__device__ __forceinline__ double rpt_residual(const RptLane &L, double X0, double X1, double X2, double (&J)[3]) {
    const double hk = ((L.pk[0] * X0 + L.pk[1] * X1) + L.pk[2] * X2) + L.pk[3];
    const double h2 = ((L.p2[0] * X0 + L.p2[1] * X1) + L.p2[2] * X2) + L.p2[3];
    const double q = hk / h2, ih = 1.0 / h2;
#pragma unroll
    for (int j = 0; j < 3; ++j) J[j] = (L.pk[j] - q * L.p2[j]) * ih;
    return q - L.o;
}

// One accumulation at X: s[0] the cost, s[1 .. 3] g = J^T (w f), s[4 .. 9] the upper triangle of H = J^T diag(w) J (00 01 02 11 12 22);
// lm.h's soft_l1 on the scalar residual.  Every lane returns the same bits.
__device__ __forceinline__ void rpt_accumulate(const RptLane &L, double X0, double X1, double X2, double f_scale, double (&s)[10]) {
    double J[3];
    const double f = rpt_residual(L, X0, X1, X2, J);
    double v[10], w;
    soft_l1(f / f_scale, v[0], w);
    const double wf = w * f;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[1 + i] = J[i] * wf;
    v[4] = (w * J[0]) * J[0]; v[5] = (w * J[0]) * J[1]; v[6] = (w * J[0]) * J[2];
    v[7] = (w * J[1]) * J[1]; v[8] = (w * J[1]) * J[2]; v[9] = (w * J[2]) * J[2];
#pragma unroll
    for (int i = 0; i < 10; ++i) s[i] = wave_sum(L.active ? v[i] : 0.0);  // selection, not multiplication: NaN * 0 is NaN
    s[0] = 0.5 * f_scale * f_scale * s[0];
}

__global__ void __launch_bounds__(64 * RPT_WAVES) k_refine_points(RefinePointsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long prob = (long long)blockIdx.x * RPT_WAVES + wave;
    if (prob >= a.NP) return;  // (wave-uniform; the kernel has no barrier)
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const RptLane L = rpt_load(a, prob, lane);
    double cur[3], cand[3], g[3] = {0.0, 0.0, 0.0}, H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Lc[9], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) cur[i] = cand[i] = a.xyz0[3 * prob + i];
    LmState st = {LM_LAMBDA0, nan, nan, 0, 0, true};
    int status = lm_status(0);

    if (rpt_views(a, prob) < 2) {
        status = SMIL_REFINE_POINTS_FEW_VIEWS;
    } else {
        for (int step = 0; step < a.max_steps; ++step) {
            double s[10];
            rpt_accumulate(L, cand[0], cand[1], cand[2], a.f_scale, s);
            int r = lm_judge(st, s[0]);
            if (r & LM_TAKE) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    cur[i] = cand[i];
                    g[i] = s[1 + i];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) H[i] = s[4 + i];
            }
            if (!(r & LM_DONE)) r |= lm_propose<3>(st, H, g, cur, cand, Lc, d);
            r = __builtin_amdgcn_readfirstlane(r);  // every lane holds the same cost, so the same result: a scalar branch
            if (r & LM_DONE) {
                status = lm_status(r);
                break;
            }
        }
    }

    if (a.view_err) {  // at the returned point; lanes 2 c and 2 c + 1 hold the two components of view c
        double J[3];
        const double f = rpt_residual(L, cur[0], cur[1], cur[2], J), fo = __shfl_xor(f, 1, 64);
        if (!(lane & 1) && (lane >> 1) < a.C) a.view_err[(size_t)prob * a.C + (lane >> 1)] = L.active ? sqrt(f * f + fo * fo) : nan;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) a.xyz[3 * prob + i] = cur[i];
        a.status[prob] = status;
        a.n_accept[prob] = st.n_accept;
        a.n_trial[prob] = st.n_trial;
        a.cost0[prob] = st.cost0;
        a.cost[prob] = st.cost_cur;
    }
}

__global__ void __launch_bounds__(64 * RPT_WAVES) k_refine_points_evaluate(RefinePointsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long prob = (long long)blockIdx.x * RPT_WAVES + wave;
    if (prob >= a.NP) return;  // (wave-uniform)
    const RptLane L = rpt_load(a, prob, lane);
    double s[10];
    rpt_accumulate(L, a.xyz0[3 * prob], a.xyz0[3 * prob + 1], a.xyz0[3 * prob + 2], a.f_scale, s);
    if (lane == 0) {
        a.cost[prob] = s[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) a.g[3 * prob + i] = s[1 + i];
        double *H = a.H + 9 * prob;
        H[0] = s[4]; H[1] = s[5]; H[2] = s[6];
        H[3] = s[5]; H[4] = s[7]; H[5] = s[8];
        H[6] = s[6]; H[7] = s[8]; H[8] = s[9];
    }
}

// ---- host ----
// What both entry points check, in this order, before a device is touched.  *NP = N Kp; zero: nothing to do.
static int refine_points_check(const char *who, int64_t N, int32_t Kp, int32_t C, double f_scale, long long *NP) {
    SMIL_REQUIRE(C >= 1, "%s: bad size C=%d", who, C);
    if (const int rc = smil_check_views(who, C, "a problem's residuals are the lanes of one wave")) return rc;
    if (const int rc = smil_check_f_scale(who, f_scale)) return rc;
    SMIL_REQUIRE(N >= 0 && Kp >= 0, "%s: bad sizes N=%lld Kp=%d", who, (long long)N, Kp);
    if (const int rc = smil_check_grid(who, N, Kp, RPT_WAVES)) return rc;
    *NP = (long long)N * Kp;
    return SMIL_OK;
}

extern "C" int smil_refine_points_evaluate(const double *P, const double *obs, const uint32_t *view_mask, const double *xyz, int64_t N,
                                           int32_t Kp, int32_t C, double f_scale, double *cost, double *g, double *H, void *stream_) {
    RefinePointsArgs a = {};
    const int rc = refine_points_check("smil_refine_points_evaluate", N, Kp, C, f_scale, &a.NP);
    if (rc != SMIL_OK) return rc;
    if (a.NP == 0) return SMIL_OK;
    SMIL_REQUIRE(P && obs && view_mask && xyz && cost && g && H, "smil_refine_points_evaluate: null argument");
    a.P = P; a.obs = obs; a.mask = view_mask; a.xyz0 = xyz; a.C = C; a.f_scale = f_scale; a.cost = cost; a.g = g; a.H = H;
    const unsigned blocks = (unsigned)((a.NP + RPT_WAVES - 1) / RPT_WAVES);
    hipLaunchKernelGGL(k_refine_points_evaluate, dim3(blocks), dim3(64 * RPT_WAVES), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_refine_points(const double *P, const double *obs, const uint32_t *view_mask, const double *xyz0, int64_t N, int32_t Kp,
                                  int32_t C, double f_scale, int32_t max_steps, double *xyz, int32_t *status, int32_t *n_accepted,
                                  int32_t *n_trials, double *cost0, double *cost, double *view_err, void *stream_) {
    RefinePointsArgs a = {};
    const int rc = refine_points_check("smil_refine_points", N, Kp, C, f_scale, &a.NP);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(max_steps >= 1, "smil_refine_points: max_steps=%d must be >= 1", max_steps);
    if (a.NP == 0) return SMIL_OK;
    SMIL_REQUIRE(P && obs && view_mask && xyz0 && xyz && status && n_accepted && n_trials && cost0 && cost, "smil_refine_points: null argument");
    a.P = P; a.obs = obs; a.mask = view_mask; a.xyz0 = xyz0; a.C = C; a.max_steps = max_steps; a.f_scale = f_scale;
    a.xyz = xyz; a.cost0 = cost0; a.cost = cost; a.view_err = view_err;
    a.status = (int *)status; a.n_accept = (int *)n_accepted; a.n_trial = (int *)n_trials;
    const unsigned blocks = (unsigned)((a.NP + RPT_WAVES - 1) / RPT_WAVES);
    hipLaunchKernelGGL(k_refine_points, dim3(blocks), dim3(64 * RPT_WAVES), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
