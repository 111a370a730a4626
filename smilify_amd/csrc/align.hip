// Rigid and similarity alignment of 3-D keypoint sets for gfx950: which rotation, translation and scale carries src (B,J,3) onto
// dst (B,J,3) in the weighted least-squares sense - Horn's quaternion method, its closed-form gradient, the soft-L1 reweighted
// variant and the fused per-joint errors (MPJPE, PA-MPJPE).  The semantics are stated at include/smilfit.h, the per-problem
// arithmetic is csrc/align.h.
//
// An extension: the reference has no alignment.  Only the masking rule of its MPJPE is mirrored
// (smal_fitter/neuralSMIL/benchmark_model.py:287-297).
//
// Storage is T (float or double); all arithmetic is float64 and every output is rounded once.  ONE wave holds one problem: lane l
// adds joints l, l + 64, ... in that order, then wave_sum(double) (common.h: a butterfly whose result depends on the values only),
// and every lane then runs the 4 x 4 solve on the same sums.  There is no atomic and no LDS in this file, nothing synchronises
// with the host (the status is a device array), and the same input gives the same bits on every call.
//
// Grids are capped at AL_MAX_BLOCKS and every kernel strides (int64 indices): there is no cap on B or J.
#include "common.h"

#include "align.h"

#define AL_THREADS 256
#define AL_WAVES (AL_THREADS / WAVE)
#define AL_MAX_BLOCKS 2048
#define AL_SENTINEL 1e-6  // a target joint within this distance of the origin is the "no annotation" sentinel (joint errors only)

template <typename T>
__device__ __forceinline__ double al_ld(const void *p, long long i) { return (double)((const T *)p)[i]; }
template <typename T>
__device__ __forceinline__ void al_st(void *p, long long i, double v) { ((T *)p)[i] = (T)v; }

#define AL_FOR_EACH_WAVE(i, n) \
    for (long long i = (long long)blockIdx.x * AL_WAVES + (threadIdx.x >> 6); i < (n); i += (long long)gridDim.x * AL_WAVES)

// the two point sets of a launch and what weighs their joints
struct AlignIn {
    const void *src, *dst;
    const double *weights;  // (J) with weight_rows == 0, (B,J) with 1, or null: 1
    const uint8_t *mask;    // (B,J) or null
    int weight_rows, sentinel, J;
};

// The points of joint (b, j) and its base weight: weight x (mask != 0), and 0 where a coordinate of either point is not finite, the
// weight is not a positive finite number or (sentinel) the dst point is the sentinel.  A joint of weight 0 enters no sum.
template <typename T>
__device__ __forceinline__ double al_base_weight(const AlignIn &in, long long b, int j, double *xs, double *ys) {
    const long long bj = b * in.J + j;
    bool ok = !in.mask || in.mask[bj] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xs[k] = al_ld<T>(in.src, bj * 3 + k);
        ys[k] = al_ld<T>(in.dst, bj * 3 + k);
        ok = ok && isfinite(xs[k]) && isfinite(ys[k]);
    }
    if (in.sentinel) ok = ok && sqrt(ys[0] * ys[0] + ys[1] * ys[1] + ys[2] * ys[2]) > AL_SENTINEL;
    const double w = in.weights ? in.weights[in.weight_rows ? bj : (long long)j] : 1.0;
    return (ok && w > 0.0 && isfinite(w)) ? w : 0.0;
}

// s R x + t - y
__device__ __forceinline__ void al_residual(const AlignTransform &x, const double *xs, const double *ys, double *r) {
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = x.s * (x.R[3 * a] * xs[0] + x.R[3 * a + 1] * xs[1] + x.R[3 * a + 2] * xs[2]) + x.t[a] - ys[a];
}

// the weight a solve uses: the base weight, or with `reweigh` its soft-L1 reweighting under `prev`, the transform of the solve before
template <typename T>
__device__ __forceinline__ double al_weight(const AlignIn &in, long long b, int j, bool reweigh, const AlignTransform &prev, double inv_f2,
                                            double *xs, double *ys) {
    double w = al_base_weight<T>(in, b, j, xs, ys);
    if (reweigh && w > 0.0) {
        double r[3];
        al_residual(prev, xs, ys, r);
        w /= sqrt(1.0 + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * inv_f2);
    }
    return w;
}

// the moments of problem b in two passes: the weighted means, then the sums over the centred points
template <typename T>
__device__ __forceinline__ void al_moments(const AlignIn &in, long long b, int lane, bool reweigh, const AlignTransform &prev, double inv_f2,
                                           AlignMoments &m) {
    double acc[10], xs[3], ys[3];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = 0.0;
    for (int j = lane; j < in.J; j += WAVE) {
        const double w = al_weight<T>(in, b, j, reweigh, prev, inv_f2, xs, ys);
        if (!(w > 0.0)) continue;
        acc[0] += w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[1 + k] += w * xs[k];
            acc[4 + k] += w * ys[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = wave_sum(acc[k]);
    m.W = acc[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m.mx[k] = m.W > 0.0 ? acc[1 + k] / m.W : 0.0;
        m.my[k] = m.W > 0.0 ? acc[4 + k] / m.W : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int j = lane; j < in.J; j += WAVE) {
        const double w = al_weight<T>(in, b, j, reweigh, prev, inv_f2, xs, ys);
        if (!(w > 0.0)) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            xs[k] -= m.mx[k];
            ys[k] -= m.my[k];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * a + c] += w * xs[a] * ys[c];
        acc[9] += w * (xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2]);
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = wave_sum(acc[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) m.M[k] = acc[k];
    m.vx = acc[9];
}

// what the forward keeps per problem for the backward, float64 (SMIL_ALIGN_SAVED values)
#define AL_SV_LAM 0   // 4 eigenvalues, descending
#define AL_SV_VEC 4   // 16: their eigenvectors, the first is q
#define AL_SV_MX 20   // 3
#define AL_SV_MY 23   // 3
#define AL_SV_M 26    // 9
#define AL_SV_VX 35
#define AL_SV_S 36
#define AL_SV_W 37
static_assert(AL_SV_W < SMIL_ALIGN_SAVED, "the saved record is larger than the header says");

template <typename T>
__global__ void __launch_bounds__(AL_THREADS) k_align_forward(AlignIn in, long long B, int with_scale, double min_gap, int robust_iters,
                                                               double inv_f2, void *R, void *t, void *s, int32_t *status, void *gap,
                                                               void *rms, double *w_final, double *saved) {
    const int lane = threadIdx.x & 63;
    AL_FOR_EACH_WAVE(b, B) {
        AlignMoments m;
        AlignEig e;
        AlignTransform x = {}, prev = {};
        for (int it = 0; it <= robust_iters; ++it) {  // the plain solve, then the reweighted ones
            prev = x;
            al_moments<T>(in, b, lane, it > 0, prev, inv_f2, m);
            align_solve(m, with_scale, min_gap, e, x);
        }
        // the weights of the last solve, and its residual over the centred points
        double ss = 0.0;
        for (int j = lane; j < in.J; j += WAVE) {
            double xs[3], ys[3];
            const double w = al_weight<T>(in, b, j, robust_iters > 0, prev, inv_f2, xs, ys);
            if (w_final) w_final[b * in.J + j] = w;
            if (!(w > 0.0)) continue;
            double r2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) xs[k] -= m.mx[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double r = x.s * (x.R[3 * a] * xs[0] + x.R[3 * a + 1] * xs[1] + x.R[3 * a + 2] * xs[2]) - (ys[a] - m.my[a]);
                r2 += r * r;
            }
            ss += w * r2;
        }
        ss = wave_sum(ss);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) al_st<T>(R, b * 9 + k, x.R[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) al_st<T>(t, b * 3 + k, x.t[k]);
            al_st<T>(s, b, x.s);
            status[b] = x.status;
            al_st<T>(gap, b, x.gap);
            al_st<T>(rms, b, m.W > 0.0 ? sqrt(ss / m.W) : 0.0);
            if (saved) {
                double *sv = saved + b * SMIL_ALIGN_SAVED;
#pragma unroll
                for (int k = 0; k < 4; ++k) sv[AL_SV_LAM + k] = e.lam[k];
#pragma unroll
                for (int k = 0; k < 16; ++k) sv[AL_SV_VEC + k] = e.v[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    sv[AL_SV_MX + k] = m.mx[k];
                    sv[AL_SV_MY + k] = m.my[k];
                }
#pragma unroll
                for (int k = 0; k < 9; ++k) sv[AL_SV_M + k] = m.M[k];
                sv[AL_SV_VX] = m.vx;
                sv[AL_SV_S] = x.s;
                sv[AL_SV_W] = m.W;
            }
        }
    }
}

// d src and / or d dst (either null) from the upstream gR (B,9), gt (B,3), gs (B), any of them null (zero)
template <typename T>
__global__ void __launch_bounds__(AL_THREADS) k_align_backward(const void *src, const void *dst, const double *w_final, const double *saved,
                                                                const int32_t *status, const void *gR, const void *gt, const void *gs,
                                                                long long B, int J, int with_scale, void *dsrc, void *ddst) {
    const int lane = threadIdx.x & 63;
    AL_FOR_EACH_WAVE(b, B) {
        const bool live = status[b] == SMIL_ALIGN_OK;
        double gM[9], g_mx[3], g_my[3], mx[3], my[3], g_vx = 0.0, W = 1.0;
        if (live) {
            const double *sv = saved + b * SMIL_ALIGN_SAVED;
            AlignEig e;
            double M[9], uR[9], ut[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) e.lam[k] = sv[AL_SV_LAM + k];
#pragma unroll
            for (int k = 0; k < 16; ++k) e.v[k] = sv[AL_SV_VEC + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mx[k] = sv[AL_SV_MX + k];
                my[k] = sv[AL_SV_MY + k];
                ut[k] = gt ? al_ld<T>(gt, b * 3 + k) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                M[k] = sv[AL_SV_M + k];
                uR[k] = gR ? al_ld<T>(gR, b * 9 + k) : 0.0;
            }
            W = sv[AL_SV_W];
            align_solve_backward(e, mx, M, sv[AL_SV_VX], sv[AL_SV_S], with_scale, uR, ut, (gs && with_scale) ? al_ld<T>(gs, b) : 0.0, gM, g_vx,
                                 g_mx, g_my);
        }
        for (int j = lane; j < J; j += WAVE) {
            const long long bj = b * J + j;
            double ds[3] = {0.0, 0.0, 0.0}, dd[3] = {0.0, 0.0, 0.0};
            const double w = live ? w_final[bj] : 0.0;
            if (w > 0.0) {
                double xs[3], ys[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    xs[k] = al_ld<T>(src, bj * 3 + k) - mx[k];
                    ys[k] = al_ld<T>(dst, bj * 3 + k) - my[k];
                }
                const double wW = w / W;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    ds[a] = w * (gM[3 * a] * ys[0] + gM[3 * a + 1] * ys[1] + gM[3 * a + 2] * ys[2] + 2.0 * g_vx * xs[a]) + wW * g_mx[a];
                    dd[a] = w * (gM[a] * xs[0] + gM[3 + a] * xs[1] + gM[6 + a] * xs[2]) + wW * g_my[a];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (dsrc) al_st<T>(dsrc, bj * 3 + k, ds[k]);
                if (ddst) al_st<T>(ddst, bj * 3 + k, dd[k]);
            }
        }
    }
}

// dist (B,J), valid (B,J), status (B) of pred against target under the alignment `mode`, the valid joints as weights
template <typename T>
__global__ void __launch_bounds__(AL_THREADS) k_align_errors(AlignIn in, long long B, int mode, double scale, double min_gap, void *dist,
                                                              uint8_t *valid, int32_t *status) {
    const int lane = threadIdx.x & 63;
    AL_FOR_EACH_WAVE(b, B) {
        AlignTransform x;
        AlignMoments m;
        double count = 0.0;
        if (mode != SMIL_ALIGN_NONE) {
            AlignEig e;
            al_moments<T>(in, b, lane, false, x, 0.0, m);
            align_solve(m, mode == SMIL_ALIGN_SIMILARITY, min_gap, e, x);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) x.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
            x.s = 1.0;
            m.mx[0] = m.mx[1] = m.mx[2] = m.my[0] = m.my[1] = m.my[2] = 0.0;
        }
        for (int j = lane; j < in.J; j += WAVE) {
            double xs[3], ys[3], d = 0.0;
            const bool ok = al_base_weight<T>(in, b, j, xs, ys) > 0.0;
            if (ok) {
                // s R p + t - y with t = my - s R mx, taken over the centred points: no cancellation against the cloud's offset
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) xs[k] -= m.mx[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double r = x.s * (x.R[3 * a] * xs[0] + x.R[3 * a + 1] * xs[1] + x.R[3 * a + 2] * xs[2]) - (ys[a] - m.my[a]);
                    r2 += r * r;
                }
                d = scale * sqrt(r2);
                count += 1.0;
            }
            al_st<T>(dist, b * in.J + j, d);
            valid[b * in.J + j] = ok;
        }
        if (mode == SMIL_ALIGN_NONE) x.status = wave_sum(count) > 0.0 ? SMIL_ALIGN_OK : SMIL_ALIGN_EMPTY;
        if (lane == 0) status[b] = x.status;
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static inline dim3 al_grid(long long problems) {
    return dim3((unsigned)std::max<long long>(1, std::min<long long>(AL_MAX_BLOCKS, (problems + AL_WAVES - 1) / AL_WAVES)));
}

static int al_check(const char *who, int64_t B, int32_t J, int32_t dtype) {
    SMIL_REQUIRE(B >= 0 && J >= 0, "%s: B=%lld J=%d must not be negative", who, (long long)B, J);
    SMIL_REQUIRE(J == 0 || B <= (int64_t)0x7FFFFFFFFFFFFFFFLL / 64 / J, "%s: B J = %lld x %d overflows", who, (long long)B, J);
    SMIL_REQUIRE(dtype == SMIL_ROT_F32 || dtype == SMIL_ROT_F64, "%s: unknown dtype %d (SMIL_ROT_F32 or SMIL_ROT_F64)", who, dtype);
    return SMIL_OK;
}
static int al_check_min_gap(const char *who, double min_gap) {
    SMIL_REQUIRE(min_gap >= 0.0 && std::isfinite(min_gap), "%s: min_gap=%g must be finite and not negative", who, min_gap);
    return SMIL_OK;
}

#define AL_LAUNCH(kernel, grid, ...)                                                                          \
    do {                                                                                                      \
        if (dtype == SMIL_ROT_F32)                                                                            \
            hipLaunchKernelGGL(kernel<float>, grid, dim3(AL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);   \
        else                                                                                                  \
            hipLaunchKernelGGL(kernel<double>, grid, dim3(AL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);  \
        SMIL_LAUNCH_CHECK();                                                                                  \
    } while (0)

extern "C" int smil_align_forward(const void *src, const void *dst, const double *weights, int32_t weight_rows, const uint8_t *mask, int64_t B,
                                  int32_t J, int32_t with_scale, double min_gap, int32_t robust_iters, double robust_scale, int32_t dtype,
                                  void *R, void *t, void *s, int32_t *status, void *gap, void *rms, double *w_final, double *saved,
                                  void *stream) {
    const char *who = "smil_align_forward";
    int rc = al_check(who, B, J, dtype);
    if (rc != SMIL_OK || (rc = al_check_min_gap(who, min_gap)) != SMIL_OK) return rc;
    SMIL_REQUIRE(robust_iters >= 0, "%s: robust_iters=%d must not be negative", who, robust_iters);
    SMIL_REQUIRE(robust_iters == 0 || (robust_scale > 0.0 && std::isfinite(robust_scale)), "%s: robust_scale=%g must be positive and finite", who,
                 robust_scale);
    SMIL_REQUIRE(weight_rows == 0 || weight_rows == 1, "%s: weight_rows=%d must be 0 (J) or 1 (B,J)", who, weight_rows);
    if (B == 0) return SMIL_OK;
    SMIL_REQUIRE(R && t && s && status && gap && rms && (J == 0 || (src && dst)), "%s: null argument", who);
    const AlignIn in = {src, dst, weights, mask, weight_rows, 0, J};
    AL_LAUNCH(k_align_forward, al_grid(B), in, (long long)B, with_scale ? 1 : 0, min_gap, robust_iters,
              robust_iters > 0 ? 1.0 / (robust_scale * robust_scale) : 0.0, R, t, s, status, gap, rms, w_final, saved);
    return SMIL_OK;
}

extern "C" int smil_align_backward(const void *src, const void *dst, const double *w_final, const double *saved, const int32_t *status,
                                   const void *gR, const void *gt, const void *gs, int64_t B, int32_t J, int32_t with_scale, int32_t dtype,
                                   void *dsrc, void *ddst, void *stream) {
    const char *who = "smil_align_backward";
    const int rc = al_check(who, B, J, dtype);
    if (rc != SMIL_OK) return rc;
    if (B == 0 || J == 0 || !(dsrc || ddst)) return SMIL_OK;
    SMIL_REQUIRE(src && dst && w_final && saved && status, "%s: null argument", who);
    AL_LAUNCH(k_align_backward, al_grid(B), src, dst, w_final, saved, status, gR, gt, gs, (long long)B, J, with_scale ? 1 : 0, dsrc, ddst);
    return SMIL_OK;
}

extern "C" int smil_align_errors(const void *pred, const void *target, const uint8_t *mask, int64_t B, int32_t J, int32_t mode, int32_t sentinel,
                                 double scale, double min_gap, int32_t dtype, void *dist, uint8_t *valid, int32_t *status, void *stream) {
    const char *who = "smil_align_errors";
    int rc = al_check(who, B, J, dtype);
    if (rc != SMIL_OK || (rc = al_check_min_gap(who, min_gap)) != SMIL_OK) return rc;
    SMIL_REQUIRE(mode == SMIL_ALIGN_NONE || mode == SMIL_ALIGN_RIGID || mode == SMIL_ALIGN_SIMILARITY, "%s: unknown alignment %d", who, mode);
    SMIL_REQUIRE(std::isfinite(scale), "%s: scale=%g must be finite", who, scale);
    if (B == 0) return SMIL_OK;
    SMIL_REQUIRE(status && (J == 0 || (pred && target && dist && valid)), "%s: null argument", who);
    const AlignIn in = {pred, target, nullptr, mask, 0, sentinel ? 1 : 0, J};
    AL_LAUNCH(k_align_errors, al_grid(B), in, (long long)B, mode, scale, min_gap, dist, valid, status);
    return SMIL_OK;
}
