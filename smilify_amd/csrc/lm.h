// The robust Levenberg-Marquardt of the multi-view kernels, stated ONCE: the camera refinement (refine.hip, one host-enqueued
// (accumulate, step) pair per evaluation) and the point refinement (refine_points.hip, a loop inside the kernel) run this code, so
// they minimise the same cost under the same rules and can alternate as a bundle adjustment whose total cannot rise.  In prose:
// include/smilfit.h at smil_refine_cameras.  A caller evaluates a point, calls lm_judge, copies g and H from wherever its sums live
// when told to, and calls lm_propose unless done.
#pragma once
#include <cmath>

#include "smilfit.h"

#define LM_LAMBDA0 1e-3  // lambda of the first step

// false for NaN and +-inf
__device__ __forceinline__ bool lm_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

// scipy's soft_l1 of the SCALED residual s = f / f_scale (refine.hip multiplies by 1 / f_scale, refine_points.hip divides, and the
// two round differently): rho = 2 (sqrt(1 + z) - 1), written without its cancellation, and the weight rho' of z = s^2.
__device__ __forceinline__ void soft_l1(double s, double &rho, double &w) {
    const double z = s * s, h = sqrt(1.0 + z);
    rho = 2.0 * z / (h + 1.0);
    w = 1.0 / h;
}

struct LmState {
    double lambda, cost_cur, cost0;  // cost_cur, cost0: NaN until the first evaluation
    int n_accept, n_trial;
    bool fresh;  // no evaluation yet: the next one is of the start
};

enum : int {
    LM_TAKE = 1,      // the evaluated point becomes current: the caller copies it, its g and its H
    LM_DONE = 2,      // no further evaluation
    LM_NONFINITE = 4  // (with LM_DONE) the start has no finite cost
};

// The accept / reject rule on the cost of the point just evaluated.
__device__ __forceinline__ int lm_judge(LmState &s, double cost_new) {
    const bool finite = lm_finite(cost_new);
    s.n_trial += 1;
    if (s.fresh && !finite) {
        s.cost_cur = s.cost0 = cost_new;
        return LM_DONE | LM_NONFINITE;
    }
    int r = 0;
    if (s.fresh || (finite && cost_new < s.cost_cur)) {
        r = LM_TAKE;
        if (s.fresh) {
            s.cost0 = cost_new;
            s.fresh = false;
        } else {
            s.n_accept += 1;
            s.lambda = fmax(s.lambda / 10.0, 1e-12);
            if (s.cost_cur - cost_new < 1e-12 * s.cost_cur) r |= LM_DONE;
        }
        s.cost_cur = cost_new;
    } else {
        s.lambda *= 10.0;
    }
    if (s.lambda > 1e12) r |= LM_DONE;
    return r;
}

// (H + lambda diag H) d = -g: L L^T by rows, forward and back substitution.  H is the packed upper triangle, entry (i, j >= i) at
// i N - i (i - 1) / 2 + (j - i); L has N x N entries.  False when a pivot is not positive and finite or d is not finite.
// Up to N = 4 everything unrolls (L and d of a caller's local arrays are registers); above, the loops stay loops (L and d in LDS).
template <int N>
__device__ __forceinline__ bool lm_solve(const double *H, const double *g, double lambda, double *L, double *d) {
    constexpr int U = N <= 4 ? N : 1;  // the unrolling of the outer loops: whole, or none
    bool ok = true;
#pragma unroll U
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j <= i; ++j) {
            double v = H[j * N - j * (j - 1) / 2 + (i - j)];
            if (i == j) v += lambda * v;
            for (int k = 0; k < j; ++k) v -= L[i * N + k] * L[j * N + k];
            if (i == j) {
                ok &= v > 0.0 && lm_finite(v);
                L[i * N + i] = sqrt(v);
            } else {
                L[i * N + j] = v / L[j * N + j];
            }
        }
    }
#pragma unroll U
    for (int i = 0; i < N; ++i) {
        double v = -g[i];
        for (int k = 0; k < i; ++k) v -= L[i * N + k] * d[k];
        d[i] = v / L[i * N + i];
    }
#pragma unroll U
    for (int i = N - 1; i >= 0; --i) {
        double v = d[i];
        for (int k = i + 1; k < N; ++k) v -= L[k * N + i] * d[k];
        d[i] = v / L[i * N + i];
        ok &= lm_finite(d[i]);
    }
    return ok;
}

// The next candidate from the current point, its g and H; LM_DONE when the "no step" fallback drives lambda past its limit, else 0.
template <int N>
__device__ __forceinline__ int lm_propose(LmState &s, const double *H, const double *g, const double *cur, double *cand, double *L, double *d) {
    if (lm_solve<N>(H, g, s.lambda, L, d)) {
        for (int i = 0; i < N; ++i) cand[i] = cur[i] + d[i];
        return 0;
    }
    // no step from this system: the next evaluation is of the current point again, which is a rejection
    for (int i = 0; i < N; ++i) cand[i] = cur[i];
    s.lambda *= 10.0;
    return s.lambda > 1e12 ? LM_DONE : 0;
}

// SMIL_REFINE_* of a result of lm_judge / lm_propose (0: no result yet)
__device__ __forceinline__ int lm_status(int r) {
    return r & LM_NONFINITE ? SMIL_REFINE_NONFINITE : (r & LM_DONE ? SMIL_REFINE_CONVERGED : SMIL_REFINE_STEP_LIMIT);
}
