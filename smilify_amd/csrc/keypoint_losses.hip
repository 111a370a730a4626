// The geometry half of a multi-view regressor's loss head for gfx950: masked weighted squared error over keypoint rows, projection
// of joints to per-sample, per-view FoV cameras, the two fused, and damped DLT triangulation through the same cameras - each with an
// analytic backward.  The semantics are stated at include/smilfit.h.
//
// Replaces (reference): smal_fitter/neuralSMIL/multiview_smil_regressor.py:1623-1838 and :2250-2388, the per-sample loops of
// smil_image_regressor.py:3032-3115 and :3334-3407 and the consistency term at multiview_smil_regressor.py:1050-1110.
//
// Storage is T (float or double); all arithmetic is float64, tan included.  Nothing is kept between a forward and its backward but
// what the entry point names: a backward kernel takes the forward's inputs and recomputes.
//
// Sums.  There is no atomic in this file.  A sum over joints is taken by ONE wave: lane l adds joints l, l + 64, ... in that order,
// then wave_sum(double) (common.h: a butterfly whose result depends on the values only).  The sum over samples is taken by ONE
// workgroup of KP_THREADS threads over the per-sample partials: thread t adds samples t, t + KP_THREADS, ..., wave_sum, then the
// KP_WAVES wave sums in wave order.  Neither order depends on the grid, so the same inputs give the same bits on every call.
//
// Grids are capped at KP_MAX_BLOCKS and every kernel strides (int64 indices): there is no cap on B, V or J.
#include "common.h"

#define KP_THREADS 256
#define KP_WAVES (KP_THREADS / WAVE)
#define KP_MAX_BLOCKS 2048
#define KP_EPS 1e-8

template <typename T>
__device__ __forceinline__ double kp_ld(const void *p, long long i) { return (double)((const T *)p)[i]; }
template <typename T>
__device__ __forceinline__ void kp_st(void *p, long long i, double v) { ((T *)p)[i] = (T)v; }

// one thread per item / one wave per item, grid-stride
#define KP_FOR_EACH(i, n) \
    for (long long i = (long long)blockIdx.x * KP_THREADS + threadIdx.x; i < (n); i += (long long)gridDim.x * KP_THREADS)
#define KP_FOR_EACH_WAVE(i, n) \
    for (long long i = (long long)blockIdx.x * KP_WAVES + (threadIdx.x >> 6); i < (n); i += (long long)gridDim.x * KP_WAVES)

// ---- the camera of one (sample, view), float64 ---------------------------------------------------------------------------------
struct KpCam {
    double R[9], T[3], k00, k11, asp;
};

template <typename T>
__device__ __forceinline__ void kp_load_cam(const void *R, const void *Tr, const void *fov, const void *aspect, long long bv, KpCam &c) {
#pragma unroll
    for (int k = 0; k < 9; ++k) c.R[k] = kp_ld<T>(R, bv * 9 + k);
#pragma unroll
    for (int k = 0; k < 3; ++k) c.T[k] = kp_ld<T>(Tr, bv * 3 + k);
    c.asp = aspect ? kp_ld<T>(aspect, bv) : 1.0;
    c.k11 = 1.0 / tan(kp_ld<T>(fov, bv) * (3.14159265358979323846 / 360.0));
    c.k00 = c.k11 / c.asp;
}
// d k11 / d fov (degrees): k11 = cot(h), h = fov pi / 360
__device__ __forceinline__ double kp_dk11_dfov(const KpCam &c) { return -(1.0 + c.k11 * c.k11) * (3.14159265358979323846 / 360.0); }

struct KpProj {
    double vx, vy, vz, xn, yn;
    double u[2];  // (y, x) / (S + 1e-8) before the clamp
    double o[2];  // clamped to [0, 1]
};

__device__ __forceinline__ double kp_clamp01(double u) { return u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u); }  // (a NaN stays one, as torch.clamp)

__device__ __forceinline__ void kp_project(const KpCam &c, const double *X, double S, KpProj &p) {
    p.vx = X[0] * c.R[0] + X[1] * c.R[3] + X[2] * c.R[6] + c.T[0];
    p.vy = X[0] * c.R[1] + X[1] * c.R[4] + X[2] * c.R[7] + c.T[1];
    p.vz = X[0] * c.R[2] + X[1] * c.R[5] + X[2] * c.R[8] + c.T[2];
    p.xn = c.k00 * p.vx / p.vz;
    p.yn = c.k11 * p.vy / p.vz;
    const double hS = 0.5 * S, inv = 1.0 / (S + KP_EPS);
    p.u[0] = (hS - hS * p.yn) * inv;
    p.u[1] = (hS - hS * p.xn) * inv;
    p.o[0] = kp_clamp01(p.u[0]);
    p.o[1] = kp_clamp01(p.u[1]);
}

// gradient g on the clamped (y, x) output -> gradient dv on the view-space point, the joint's share of d k11 returned
__device__ __forceinline__ double kp_project_bwd(const KpCam &c, const KpProj &p, double S, const double *g, double *dv) {
    const double s = -(0.5 * S) / (S + KP_EPS);
    const double gyn = (p.u[0] >= 0.0 && p.u[0] <= 1.0) ? g[0] * s : 0.0;
    const double gxn = (p.u[1] >= 0.0 && p.u[1] <= 1.0) ? g[1] * s : 0.0;
    const double iz = 1.0 / p.vz;
    dv[0] = gxn * c.k00 * iz;
    dv[1] = gyn * c.k11 * iz;
    dv[2] = -(gxn * p.xn + gyn * p.yn) * iz;
    return gyn * p.vy * iz + gxn * p.vx * iz / c.asp;
}

// ---- (a) the squared-error family ----------------------------------------------------------------------------------------------
// One joint of one selected sample: is it valid under `flags`, and its target t[D].  p[D] is the prediction as stored.
template <typename T>
__device__ __forceinline__ bool kp_joint_valid(const void *target, const uint8_t *vis, long long nj, int D, int flags, const double *p, double *t) {
    bool valid = !vis || vis[nj] != 0;
    double sum_abs = 0.0;
    for (int d = 0; d < D; ++d) {
        t[d] = kp_ld<T>(target, nj * D + d);
        if (flags & SMIL_KP_TARGET_IN_UNIT) valid = valid && t[d] >= 0.0 && t[d] <= 1.0;
        if (flags & SMIL_KP_FINITE_NONZERO) valid = valid && isfinite(t[d]) && isfinite(p[d]);
        sum_abs += fabs(t[d]);
    }
    if (flags & SMIL_KP_FINITE_NONZERO) valid = valid && sum_abs > 0.0;
    return valid;
}
// the prediction as the sum reads it, and whether that coordinate takes a gradient
__device__ __forceinline__ double kp_pred(double p, int flags, bool &live) {
    live = !(flags & SMIL_KP_PRED_NAN_TO_ZERO) || isfinite(p);
    return live ? p : 0.0;
}

// per-sample partials (N,4): numerator, weighted count, valid joints, selected (0 / 1)
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_se_partials(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask,
                                                                 const double *w, long long N, int J, int D, int flags, double *part) {
    const int lane = threadIdx.x & 63;
    KP_FOR_EACH_WAVE(n, N) {
        const bool sel = !mask || mask[n] != 0;
        double num = 0.0, cnt = 0.0, nv = 0.0;
        if (sel) {
            for (int j = lane; j < J; j += WAVE) {
                const long long nj = n * J + j;
                double p[3], t[3];
                for (int d = 0; d < D; ++d) p[d] = kp_ld<T>(pred, nj * D + d);
                if (!kp_joint_valid<T>(target, vis, nj, D, flags, p, t)) continue;
                const double wj = w ? w[j] : 1.0;
                double e = 0.0;
                for (int d = 0; d < D; ++d) {
                    bool live;
                    const double diff = kp_pred(p[d], flags, live) - t[d];
                    e += diff * diff;
                }
                num += wj * e;
                cnt += wj;
                nv += 1.0;
            }
        }
        num = wave_sum(num);
        cnt = wave_sum(cnt);
        nv = wave_sum(nv);
        if (lane == 0) {
            part[4 * n + 0] = num;
            part[4 * n + 1] = cnt;
            part[4 * n + 2] = nv;
            part[4 * n + 3] = sel ? 1.0 : 0.0;
        }
    }
}

__device__ __forceinline__ double kp_block_sum(double v, double *s /* KP_WAVES */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int k = 0; k < KP_WAVES; ++k) r += s[k];
    return r;
}

// does sample n enter a per-sample mean, and its ratio num / (D cnt + eps)
__device__ __forceinline__ bool kp_sample_in(const double *part, long long n, int rule) {
    return rule == SMIL_KP_VALID_SAMPLES ? part[4 * n + 2] > 0.0 : part[4 * n + 3] > 0.0;
}

// ONE workgroup: the loss and the factor of every sample (d loss / d num_n)
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_se_final(const double *part, long long N, int D, int rule, int flags, double *factor,
                                                              void *loss) {
    __shared__ double s[KP_WAVES];
    double a = 0.0, b = 0.0, c = 0.0;
    for (long long n = threadIdx.x; n < N; n += KP_THREADS) {
        if (rule == SMIL_KP_POOLED) {
            a += part[4 * n];
            b += part[4 * n + 1];
        } else if (kp_sample_in(part, n, rule)) {
            a += part[4 * n] / ((double)D * part[4 * n + 1] + KP_EPS);
            b += 1.0;
        }
        c += part[4 * n + 2];
    }
    a = kp_block_sum(a, s);
    b = kp_block_sum(b, s);
    c = kp_block_sum(c, s);
    double value, pooled = 0.0;
    if (rule == SMIL_KP_POOLED) {
        pooled = 1.0 / ((double)D * b + KP_EPS);
        value = (flags & SMIL_KP_NO_TRAILING_EPS) ? (c > 0.0 ? a * pooled : KP_EPS) : a * pooled + KP_EPS;
    } else {
        value = (b > 0.0 ? a / b : 0.0) + KP_EPS;
    }
    if (threadIdx.x == 0) kp_st<T>(loss, 0, value);
    for (long long n = threadIdx.x; n < N; n += KP_THREADS) {
        if (rule == SMIL_KP_POOLED)
            factor[n] = pooled;
        else
            factor[n] = kp_sample_in(part, n, rule) ? 1.0 / (((double)D * part[4 * n + 1] + KP_EPS) * b) : 0.0;
    }
}

template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_se_bwd(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask,
                                                            const double *w, const double *factor, const void *up, void *dpred, long long N,
                                                            int J, int D, int flags) {
    const double upstream = kp_ld<T>(up, 0);
    KP_FOR_EACH(nj, N * J) {
        const long long n = nj / J;
        const int j = (int)(nj - n * J);
        double p[3], t[3], g[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) p[d] = kp_ld<T>(pred, nj * D + d);
        if ((!mask || mask[n] != 0) && kp_joint_valid<T>(target, vis, nj, D, flags, p, t)) {
            const double f = upstream * factor[n] * 2.0 * (w ? w[j] : 1.0);
            for (int d = 0; d < D; ++d) {
                bool live;
                const double diff = kp_pred(p[d], flags, live) - t[d];
                g[d] = live ? f * diff : 0.0;
            }
        }
        for (int d = 0; d < D; ++d) kp_st<T>(dpred, nj * D + d, g[d]);
    }
}

// ---- (b) projection ------------------------------------------------------------------------------------------------------------
// The per-point kernels (k_kp_project, k_kp_project_bwd_joints, kp_dlt_system) load a camera's thirteen values and evaluate its
// float64 tan once per point, or per (point, view): redundant work that the one-wave-per-(b, v) kernels do once per wave.  It is
// left so because a call at the sizes these losses run at (tens of thousands of points) is bound by its launches, not by this; a
// (B,V) table of k00, k11 from a kernel of its own would remove it at the price of one more launch per call.
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_project(const void *joints, const void *R, const void *Tr, const void *fov, const void *aspect,
                                                             long long B, int V, int J, double S, void *out) {
    KP_FOR_EACH(i, B * V * J) {
        const long long bv = i / J, b = bv / V;
        const int j = (int)(i - bv * J);
        KpCam c;
        KpProj p;
        double X[3];
        kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
        for (int k = 0; k < 3; ++k) X[k] = kp_ld<T>(joints, (b * J + j) * 3 + k);
        kp_project(c, X, S, p);
        kp_st<T>(out, i * 2, p.o[0]);
        kp_st<T>(out, i * 2 + 1, p.o[1]);
    }
}

// Where the gradient on a projected joint comes from: the caller's array (dout), or the pooled 2-D loss of (c) at that joint.
struct KpUpstream {
    const void *dout;  // (B,V,J,2), read where `up` is null
    const void *target;  // the loss, read where `up` (its upstream scalar) is not null
    const uint8_t *vis, *mask;
    const double *w, *factor;
    const void *up;
};
#define KP_LOSS_2D_FLAGS (SMIL_KP_TARGET_IN_UNIT | SMIL_KP_PRED_NAN_TO_ZERO)

template <typename T>
__device__ __forceinline__ void kp_upstream(const KpUpstream &s, double upstream, long long bv, int J, int j, const double *o, double *g) {
    const long long nj = bv * J + j;
    if (!s.up) {
        g[0] = kp_ld<T>(s.dout, nj * 2);
        g[1] = kp_ld<T>(s.dout, nj * 2 + 1);
        return;
    }
    double t[2];
    g[0] = g[1] = 0.0;
    if ((!s.mask || s.mask[bv] != 0) && kp_joint_valid<T>(s.target, s.vis, nj, 2, KP_LOSS_2D_FLAGS, o, t)) {
        const double f = upstream * s.factor[bv] * 2.0 * (s.w ? s.w[j] : 1.0);
        for (int d = 0; d < 2; ++d) {
            bool live;
            const double diff = kp_pred(o[d], KP_LOSS_2D_FLAGS, live) - t[d];
            g[d] = live ? f * diff : 0.0;
        }
    }
}

// one wave per (b, v): d R (9), d T (3), d fov summed over the joints
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_project_bwd_cam(const void *joints, const void *R, const void *Tr, const void *fov,
                                                                     const void *aspect, KpUpstream s, long long B, int V, int J, double S, void *dR,
                                                                     void *dT, void *dfov) {
    const int lane = threadIdx.x & 63;
    const double upstream = s.up ? kp_ld<T>(s.up, 0) : 0.0;
    KP_FOR_EACH_WAVE(bv, B * V) {
        const long long b = bv / V;
        KpCam c;
        kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
        double acc[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) acc[k] = 0.0;
        for (int j = lane; j < J; j += WAVE) {
            KpProj p;
            double X[3], g[2], dv[3];
            for (int k = 0; k < 3; ++k) X[k] = kp_ld<T>(joints, (b * J + j) * 3 + k);
            kp_project(c, X, S, p);
            kp_upstream<T>(s, upstream, bv, J, j, p.o, g);
            acc[12] += kp_project_bwd(c, p, S, g, dv);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[3 * r + q] += X[r] * dv[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[9 + q] += dv[q];
        }
#pragma unroll
        for (int k = 0; k < 13; ++k) acc[k] = wave_sum(acc[k]);
        if (lane == 0) {
            if (dR)
                for (int k = 0; k < 9; ++k) kp_st<T>(dR, bv * 9 + k, acc[k]);
            if (dT)
                for (int k = 0; k < 3; ++k) kp_st<T>(dT, bv * 3 + k, acc[9 + k]);
            if (dfov) kp_st<T>(dfov, bv, acc[12] * kp_dk11_dfov(c));
        }
    }
}

// one thread per (b, j): d joints summed over the views in view order
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_project_bwd_joints(const void *joints, const void *R, const void *Tr, const void *fov,
                                                                        const void *aspect, KpUpstream s, long long B, int V, int J, double S,
                                                                        void *djoints) {
    const double upstream = s.up ? kp_ld<T>(s.up, 0) : 0.0;
    KP_FOR_EACH(bj, B * J) {
        const long long b = bj / J;
        const int j = (int)(bj - b * J);
        double X[3], gX[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k) X[k] = kp_ld<T>(joints, bj * 3 + k);
        for (int v = 0; v < V; ++v) {
            const long long bv = b * V + v;
            KpCam c;
            KpProj p;
            double g[2], dv[3];
            kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
            kp_project(c, X, S, p);
            kp_upstream<T>(s, upstream, bv, J, j, p.o, g);
            kp_project_bwd(c, p, S, g, dv);
#pragma unroll
            for (int r = 0; r < 3; ++r) gX[r] += c.R[3 * r] * dv[0] + c.R[3 * r + 1] * dv[1] + c.R[3 * r + 2] * dv[2];
        }
        for (int k = 0; k < 3; ++k) kp_st<T>(djoints, bj * 3 + k, gX[k]);
    }
}

// ---- (c) projection and pooled 2-D loss, the projected array never written: the partials of k_kp_se_partials per (b, v) ----------
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_project_loss_partials(const void *joints, const void *R, const void *Tr, const void *fov,
                                                                           const void *aspect, const void *target, const uint8_t *vis,
                                                                           const uint8_t *mask, const double *w, long long B, int V, int J, double S,
                                                                           double *part) {
    const int lane = threadIdx.x & 63;
    KP_FOR_EACH_WAVE(bv, B * V) {
        const long long b = bv / V;
        const bool sel = !mask || mask[bv] != 0;
        double num = 0.0, cnt = 0.0, nv = 0.0;
        if (sel) {
            KpCam c;
            kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
            for (int j = lane; j < J; j += WAVE) {
                KpProj p;
                double X[3], t[2];
                for (int k = 0; k < 3; ++k) X[k] = kp_ld<T>(joints, (b * J + j) * 3 + k);
                kp_project(c, X, S, p);
                if (!kp_joint_valid<T>(target, vis, bv * J + j, 2, KP_LOSS_2D_FLAGS, p.o, t)) continue;
                const double wj = w ? w[j] : 1.0;
                double e = 0.0;
                for (int d = 0; d < 2; ++d) {
                    bool live;
                    const double diff = kp_pred(p.o[d], KP_LOSS_2D_FLAGS, live) - t[d];
                    e += diff * diff;
                }
                num += wj * e;
                cnt += wj;
                nv += 1.0;
            }
        }
        num = wave_sum(num);
        cnt = wave_sum(cnt);
        nv = wave_sum(nv);
        if (lane == 0) {
            part[4 * bv + 0] = num;
            part[4 * bv + 1] = cnt;
            part[4 * bv + 2] = nv;
            part[4 * bv + 3] = sel ? 1.0 : 0.0;
        }
    }
}

// ---- (d) damped DLT triangulation ------------------------------------------------------------------------------------------------
// The two rows of one visible (view, joint): a[0..2] the xyz part, a[3] the w part.
__device__ __forceinline__ void kp_dlt_rows(const KpCam &c, double ky, double kx, double S, double &u, double &v, double *a1, double *a2) {
    u = 1.0 - (kx * S) / (0.5 * S);
    v = 1.0 - (ky * S) / (0.5 * S);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a1[i] = u * c.R[3 * i + 2] - c.k00 * c.R[3 * i];
        a2[i] = v * c.R[3 * i + 2] - c.k11 * c.R[3 * i + 1];
    }
    a1[3] = u * c.T[2] - c.k00 * c.T[0];
    a2[3] = v * c.T[2] - c.k11 * c.T[1];
}

// Cholesky factor of the symmetric M = (m00, m10, m11, m20, m21, m22), in place
__device__ __forceinline__ void kp_chol3(double *m) {
    m[0] = sqrt(m[0]);
    m[1] /= m[0];
    m[3] /= m[0];
    m[2] = sqrt(m[2] - m[1] * m[1]);
    m[4] = (m[4] - m[3] * m[1]) / m[2];
    m[5] = sqrt(m[5] - m[3] * m[3] - m[4] * m[4]);
}
__device__ __forceinline__ void kp_chol3_solve(const double *l, const double *rhs, double *x) {
    const double y0 = rhs[0] / l[0];
    const double y1 = (rhs[1] - l[1] * y0) / l[2];
    const double y2 = (rhs[2] - l[3] * y0 - l[4] * y1) / l[5];
    x[2] = y2 / l[5];
    x[1] = (y1 - l[4] * x[2]) / l[2];
    x[0] = (y0 - l[1] * x[1] - l[3] * x[2]) / l[0];
}

// the system of joint (b, j): Cholesky factor of M + damping I in m[6], c[3], the number of views that see it
template <typename T>
__device__ __forceinline__ int kp_dlt_system(const void *kp, const uint8_t *vis, const uint8_t *vmask, const void *R, const void *Tr,
                                             const void *fov, const void *aspect, long long b, int V, int J, int j, double S, double damping,
                                             double *m, double *cv) {
    int count = 0;
    for (int k = 0; k < 6; ++k) m[k] = 0.0;
    for (int k = 0; k < 3; ++k) cv[k] = 0.0;
    for (int v = 0; v < V; ++v) {
        const long long bv = b * V + v, nj = bv * J + j;
        if ((vmask && vmask[bv] == 0) || (vis && vis[nj] == 0)) continue;
        KpCam c;
        double uu, vv, a1[4], a2[4];
        kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
        kp_dlt_rows(c, kp_ld<T>(kp, nj * 2), kp_ld<T>(kp, nj * 2 + 1), S, uu, vv, a1, a2);
        m[0] += a1[0] * a1[0] + a2[0] * a2[0];
        m[1] += a1[1] * a1[0] + a2[1] * a2[0];
        m[2] += a1[1] * a1[1] + a2[1] * a2[1];
        m[3] += a1[2] * a1[0] + a2[2] * a2[0];
        m[4] += a1[2] * a1[1] + a2[2] * a2[1];
        m[5] += a1[2] * a1[2] + a2[2] * a2[2];
        for (int k = 0; k < 3; ++k) cv[k] -= a1[k] * a1[3] + a2[k] * a2[3];
        ++count;
    }
    m[0] += damping;
    m[2] += damping;
    m[5] += damping;
    kp_chol3(m);
    return count;
}

template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_triangulate(const void *kp, const uint8_t *vis, const uint8_t *vmask, const void *R,
                                                                 const void *Tr, const void *fov, const void *aspect, long long B, int V, int J,
                                                                 double S, double damping, double max_norm, void *points, uint8_t *valid,
                                                                 uint8_t *sane) {
    KP_FOR_EACH(bj, B * J) {
        const long long b = bj / J;
        const int j = (int)(bj - b * J);
        double m[6], cv[3], p[3];
        const int count = kp_dlt_system<T>(kp, vis, vmask, R, Tr, fov, aspect, b, V, J, j, S, damping, m, cv);
        kp_chol3_solve(m, cv, p);
        for (int k = 0; k < 3; ++k) kp_st<T>(points, bj * 3 + k, p[k]);
        if (valid) valid[bj] = count >= 2;
        if (sane) sane[bj] = count >= 2 && sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) < max_norm;
    }
}

// backward, first kernel: lambda = M^-1 g and p per (b, j) as float64 (B,J,6)
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_triangulate_bwd_solve(const void *kp, const uint8_t *vis, const uint8_t *vmask, const void *R,
                                                                           const void *Tr, const void *fov, const void *aspect, const void *dpoints,
                                                                           long long B, int V, int J, double S, double damping, double *lam_p) {
    KP_FOR_EACH(bj, B * J) {
        const long long b = bj / J;
        const int j = (int)(bj - b * J);
        double m[6], cv[3], p[3], g[3], lam[3];
        kp_dlt_system<T>(kp, vis, vmask, R, Tr, fov, aspect, b, V, J, j, S, damping, m, cv);
        kp_chol3_solve(m, cv, p);
        for (int k = 0; k < 3; ++k) g[k] = kp_ld<T>(dpoints, bj * 3 + k);
        kp_chol3_solve(m, g, lam);
        for (int k = 0; k < 3; ++k) {
            lam_p[bj * 6 + k] = lam[k];
            lam_p[bj * 6 + 3 + k] = p[k];
        }
    }
}

// backward, second kernel: one wave per (b, v), the camera gradients summed over the joints it sees
template <typename T>
__global__ void __launch_bounds__(KP_THREADS) k_kp_triangulate_bwd_cam(const void *kp, const uint8_t *vis, const uint8_t *vmask, const void *R,
                                                                         const void *Tr, const void *fov, const void *aspect, const double *lam_p,
                                                                         long long B, int V, int J, double S, void *dR, void *dT, void *dfov) {
    const int lane = threadIdx.x & 63;
    KP_FOR_EACH_WAVE(bv, B * V) {
        const long long b = bv / V;
        KpCam c;
        kp_load_cam<T>(R, Tr, fov, aspect, bv, c);
        double acc[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) acc[k] = 0.0;
        if (!vmask || vmask[bv] != 0) {
            for (int j = lane; j < J; j += WAVE) {
                const long long nj = bv * J + j;
                if (vis && vis[nj] == 0) continue;
                const double *lp = lam_p + (b * J + j) * 6;
                const double lam[3] = {lp[0], lp[1], lp[2]}, p[3] = {lp[3], lp[4], lp[5]};
                double uu, vv, a1[4], a2[4], g1[4], g2[4];
                kp_dlt_rows(c, kp_ld<T>(kp, nj * 2), kp_ld<T>(kp, nj * 2 + 1), S, uu, vv, a1, a2);
                // d a = -lambda (p . a_xyz + a_w) - p (lambda . a_xyz) on the xyz part, -(lambda . a_xyz) on the w part
                const double r1 = p[0] * a1[0] + p[1] * a1[1] + p[2] * a1[2] + a1[3], l1 = lam[0] * a1[0] + lam[1] * a1[1] + lam[2] * a1[2];
                const double r2 = p[0] * a2[0] + p[1] * a2[1] + p[2] * a2[2] + a2[3], l2 = lam[0] * a2[0] + lam[1] * a2[1] + lam[2] * a2[2];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    g1[i] = -lam[i] * r1 - p[i] * l1;
                    g2[i] = -lam[i] * r2 - p[i] * l2;
                }
                g1[3] = -l1;
                g2[3] = -l2;
                double dk00 = 0.0, dk11 = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    acc[3 * i + 2] += uu * g1[i] + vv * g2[i];
                    acc[3 * i] -= c.k00 * g1[i];
                    acc[3 * i + 1] -= c.k11 * g2[i];
                    dk00 -= g1[i] * c.R[3 * i];
                    dk11 -= g2[i] * c.R[3 * i + 1];
                }
                acc[11] += uu * g1[3] + vv * g2[3];
                acc[9] -= c.k00 * g1[3];
                acc[10] -= c.k11 * g2[3];
                dk00 -= g1[3] * c.T[0];
                dk11 -= g2[3] * c.T[1];
                acc[12] += dk11 + dk00 / c.asp;
            }
        }
#pragma unroll
        for (int k = 0; k < 13; ++k) acc[k] = wave_sum(acc[k]);
        if (lane == 0) {
            if (dR)
                for (int k = 0; k < 9; ++k) kp_st<T>(dR, bv * 9 + k, acc[k]);
            if (dT)
                for (int k = 0; k < 3; ++k) kp_st<T>(dT, bv * 3 + k, acc[9 + k]);
            if (dfov) kp_st<T>(dfov, bv, acc[12] * kp_dk11_dfov(c));
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static inline dim3 kp_grid(long long items, int per_block) {
    return dim3((unsigned)std::max<long long>(1, std::min<long long>(KP_MAX_BLOCKS, (items + per_block - 1) / per_block)));
}

static int kp_check_dtype(const char *who, int32_t dtype) {
    SMIL_REQUIRE(dtype == SMIL_ROT_F32 || dtype == SMIL_ROT_F64, "%s: unknown dtype %d (SMIL_ROT_F32 or SMIL_ROT_F64)", who, dtype);
    return SMIL_OK;
}
static int kp_check_views(const char *who, int64_t B, int32_t V, int32_t J, double S, int32_t dtype) {
    SMIL_REQUIRE(B >= 0 && V >= 0 && J >= 0, "%s: B=%lld V=%d J=%d must not be negative", who, (long long)B, V, J);
    SMIL_REQUIRE(S > 0.0 && std::isfinite(S), "%s: image size %g must be positive and finite", who, S);
    SMIL_REQUIRE(V == 0 || J == 0 || B <= (int64_t)0x7FFFFFFFFFFFFFFFLL / 16 / V / J, "%s: B V J = %lld x %d x %d overflows", who, (long long)B, V, J);
    return kp_check_dtype(who, dtype);
}

// kernel<float> or kernel<double> over `grid`
#define KP_LAUNCH(kernel, grid, ...)                                                                          \
    do {                                                                                                      \
        if (dtype == SMIL_ROT_F32)                                                                            \
            hipLaunchKernelGGL(kernel<float>, grid, dim3(KP_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);   \
        else                                                                                                  \
            hipLaunchKernelGGL(kernel<double>, grid, dim3(KP_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);  \
        SMIL_LAUNCH_CHECK();                                                                                  \
    } while (0)

static int kp_check_se(const char *who, int64_t N, int32_t J, int32_t D, int32_t flags, int32_t dtype) {
    SMIL_REQUIRE(N >= 0 && J >= 0, "%s: N=%lld J=%d must not be negative", who, (long long)N, J);
    SMIL_REQUIRE(D == 2 || D == 3, "%s: D=%d must be 2 or 3", who, D);
    SMIL_REQUIRE(J == 0 || N <= (int64_t)0x7FFFFFFFFFFFFFFFLL / 16 / J, "%s: N J = %lld x %d overflows", who, (long long)N, J);
    SMIL_REQUIRE((flags & ~(SMIL_KP_TARGET_IN_UNIT | SMIL_KP_PRED_NAN_TO_ZERO | SMIL_KP_FINITE_NONZERO | SMIL_KP_NO_TRAILING_EPS)) == 0,
                 "%s: unknown flags 0x%x", who, flags);
    return kp_check_dtype(who, dtype);
}
static int kp_check_rule(const char *who, int32_t rule) {
    SMIL_REQUIRE(rule == SMIL_KP_POOLED || rule == SMIL_KP_VALID_SAMPLES || rule == SMIL_KP_SAMPLES, "%s: unknown reduction %d", who, rule);
    return SMIL_OK;
}

extern "C" int smil_kp_se_forward(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask, const double *weights, int64_t N,
                                  int32_t J, int32_t D, int32_t flags, int32_t rule, int32_t dtype, double *partials, double *factor, void *loss,
                                  void *stream) {
    const char *who = "smil_kp_se_forward";
    int rc = kp_check_se(who, N, J, D, flags, dtype);
    if (rc != SMIL_OK || (rc = kp_check_rule(who, rule)) != SMIL_OK) return rc;
    SMIL_REQUIRE(loss, "%s: null argument", who);
    SMIL_REQUIRE(N == 0 || (partials && factor && (J == 0 || (pred && target))), "%s: null argument", who);
    if (N > 0) KP_LAUNCH(k_kp_se_partials, kp_grid(N, KP_WAVES), pred, target, vis, mask, weights, (long long)N, J, D, flags, partials);
    KP_LAUNCH(k_kp_se_final, dim3(1), (const double *)partials, (long long)N, D, rule, flags, factor, loss);
    return SMIL_OK;
}

extern "C" int smil_kp_se_backward(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask, const double *weights,
                                   const double *factor, const void *upstream, void *dpred, int64_t N, int32_t J, int32_t D, int32_t flags,
                                   int32_t dtype, void *stream) {
    const char *who = "smil_kp_se_backward";
    const int rc = kp_check_se(who, N, J, D, flags, dtype);
    if (rc != SMIL_OK) return rc;
    if (N == 0 || J == 0) return SMIL_OK;
    SMIL_REQUIRE(pred && target && factor && upstream && dpred, "%s: null argument", who);
    KP_LAUNCH(k_kp_se_bwd, kp_grid(N * J, KP_THREADS), pred, target, vis, mask, weights, factor, upstream, dpred, (long long)N, J, D, flags);
    return SMIL_OK;
}

extern "C" int smil_kp_project(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, int64_t B, int32_t V,
                               int32_t J, double S, int32_t dtype, void *out, void *stream) {
    const char *who = "smil_kp_project";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    if (B == 0 || V == 0 || J == 0) return SMIL_OK;
    SMIL_REQUIRE(joints && R && T && fov && out, "%s: null argument", who);
    KP_LAUNCH(k_kp_project, kp_grid(B * V * J, KP_THREADS), joints, R, T, fov, aspect, (long long)B, V, J, S, out);
    return SMIL_OK;
}

// the two backward kernels of (b) and (c); an output nobody wants is NULL
static int kp_project_backward(const char *who, const void *joints, const void *R, const void *T, const void *fov, const void *aspect,
                               const KpUpstream &s, int64_t B, int32_t V, int32_t J, double S, int32_t dtype, void *djoints, void *dR, void *dT,
                               void *dfov, void *stream) {
    if (B == 0) return SMIL_OK;
    SMIL_REQUIRE((V == 0 || (R && T && fov)) && (J == 0 || joints), "%s: null argument", who);
    if (V > 0 && (dR || dT || dfov))
        KP_LAUNCH(k_kp_project_bwd_cam, kp_grid(B * V, KP_WAVES), joints, R, T, fov, aspect, s, (long long)B, V, J, S, dR, dT, dfov);
    if (J > 0 && djoints) KP_LAUNCH(k_kp_project_bwd_joints, kp_grid(B * J, KP_THREADS), joints, R, T, fov, aspect, s, (long long)B, V, J, S, djoints);
    return SMIL_OK;
}

extern "C" int smil_kp_project_backward(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, const void *dout,
                                        int64_t B, int32_t V, int32_t J, double S, int32_t dtype, void *djoints, void *dR, void *dT, void *dfov,
                                        void *stream) {
    const char *who = "smil_kp_project_backward";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(dout || B == 0 || V == 0 || J == 0, "%s: null argument", who);
    // (with V == 0 or J == 0 the sums are empty: the kernels write zeros and never read dout)
    KpUpstream s = {dout, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return kp_project_backward(who, joints, R, T, fov, aspect, s, B, V, J, S, dtype, djoints, dR, dT, dfov, stream);
}

extern "C" int smil_kp_project_loss(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, const void *target,
                                    const uint8_t *vis, const uint8_t *view_mask, const double *weights, int64_t B, int32_t V, int32_t J, double S,
                                    int32_t dtype, double *partials, double *factor, void *loss, void *stream) {
    const char *who = "smil_kp_project_loss";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(loss, "%s: null argument", who);
    const long long N = (long long)B * V;
    SMIL_REQUIRE(N == 0 || (partials && factor && R && T && fov && (J == 0 || (joints && target))), "%s: null argument", who);
    if (N > 0)
        KP_LAUNCH(k_kp_project_loss_partials, kp_grid(N, KP_WAVES), joints, R, T, fov, aspect, target, vis, view_mask, weights, (long long)B, V, J,
                  S, partials);
    KP_LAUNCH(k_kp_se_final, dim3(1), (const double *)partials, N, 2, SMIL_KP_POOLED, 0, factor, loss);
    return SMIL_OK;
}

extern "C" int smil_kp_project_loss_backward(const void *joints, const void *R, const void *T, const void *fov, const void *aspect,
                                             const void *target, const uint8_t *vis, const uint8_t *view_mask, const double *weights,
                                             const double *factor, const void *upstream, int64_t B, int32_t V, int32_t J, double S, int32_t dtype,
                                             void *djoints, void *dR, void *dT, void *dfov, void *stream) {
    const char *who = "smil_kp_project_loss_backward";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(B == 0 || ((V == 0 || J == 0 || target) && (V == 0 || factor) && upstream), "%s: null argument", who);
    KpUpstream s = {nullptr, target, vis, view_mask, weights, factor, upstream};
    return kp_project_backward(who, joints, R, T, fov, aspect, s, B, V, J, S, dtype, djoints, dR, dT, dfov, stream);
}

extern "C" int smil_kp_triangulate(const void *kp, const uint8_t *vis, const uint8_t *view_mask, const void *R, const void *T, const void *fov,
                                   const void *aspect, int64_t B, int32_t V, int32_t J, double S, double damping, double max_norm, int32_t dtype,
                                   void *points, uint8_t *valid, uint8_t *sane, void *stream) {
    const char *who = "smil_kp_triangulate";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(damping > 0.0 && std::isfinite(damping), "%s: damping=%g must be positive and finite (it keeps M definite for a joint seen by fewer than two views)", who, damping);
    if (B == 0 || J == 0) return SMIL_OK;
    SMIL_REQUIRE(points && (V == 0 || (kp && R && T && fov)), "%s: null argument", who);
    KP_LAUNCH(k_kp_triangulate, kp_grid(B * J, KP_THREADS), kp, vis, view_mask, R, T, fov, aspect, (long long)B, V, J, S, damping, max_norm, points,
              valid, sane);
    return SMIL_OK;
}

extern "C" int smil_kp_triangulate_backward(const void *kp, const uint8_t *vis, const uint8_t *view_mask, const void *R, const void *T,
                                            const void *fov, const void *aspect, const void *dpoints, int64_t B, int32_t V, int32_t J, double S,
                                            double damping, int32_t dtype, double *lam_p, void *dR, void *dT, void *dfov, void *stream) {
    const char *who = "smil_kp_triangulate_backward";
    const int rc = kp_check_views(who, B, V, J, S, dtype);
    if (rc != SMIL_OK) return rc;
    SMIL_REQUIRE(damping > 0.0 && std::isfinite(damping), "%s: damping=%g must be positive and finite (it keeps M definite for a joint seen by fewer than two views)", who, damping);
    if (B == 0 || V == 0 || !(dR || dT || dfov)) return SMIL_OK;
    SMIL_REQUIRE(R && T && fov && (J == 0 || (kp && dpoints && lam_p)), "%s: null argument", who);
    if (J > 0)
        KP_LAUNCH(k_kp_triangulate_bwd_solve, kp_grid(B * J, KP_THREADS), kp, vis, view_mask, R, T, fov, aspect, dpoints, (long long)B, V, J, S,
                  damping, lam_p);
    KP_LAUNCH(k_kp_triangulate_bwd_cam, kp_grid(B * V, KP_WAVES), kp, vis, view_mask, R, T, fov, aspect, (const double *)lam_p, (long long)B, V, J, S,
              dR, dT, dfov);
    return SMIL_OK;
}
