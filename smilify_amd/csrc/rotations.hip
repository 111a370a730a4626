// Rotation conversions for gfx950: 6-D <-> matrix <-> axis-angle, forward and analytic backward, and the Frobenius distance of two
// 6-D rotations.  The semantics are stated at include/smilfit.h, the arithmetic in rot.h.
//
// Replaces (reference): the four pytorch3d.transforms functions behind smal_fitter/neuralSMIL/smil_image_regressor.py:26-96 and the
// rotation losses at :2123-2163 and :3117-3266 - about forty torch launches per call, forward and backward.
//
// Every kernel has the same shape: ONE rotation per lane, a grid-stride loop over n (int64), float64 arithmetic whatever the storage
// type T (float or double).  The layout is the API's, 3, 6 or 9 contiguous values per rotation, and a lane reads and writes its own
// row with plain element accesses: rows are only element-aligned, and from that the compiler forms the widest accesses the hardware
// takes at that alignment (dwordx4 / x3 / x2 pieces of a row).  A wave's rows are one contiguous run of 64 rows, so every fetched
// line is used by the wave that fetched it.  Nothing is staged in LDS and nothing is kept between the forward and the backward:
// a backward kernel takes the forward's inputs and recomputes.
#include "common.h"
#include "rot.h"

#define ROT_THREADS 256
#define ROT_MAX_BLOCKS 2048

template <typename T, int K>
__device__ __forceinline__ void rot_load(const void *p, long long i, double (&v)[K]) {
    const T *row = (const T *)p + i * K;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (double)row[k];
}
template <typename T, int K>
__device__ __forceinline__ void rot_store(void *p, long long i, const double *v) {
    T *row = (T *)p + i * K;
#pragma unroll
    for (int k = 0; k < K; ++k) row[k] = (T)v[k];
}

#define ROT_FOR_EACH(i, n) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_rot6d_to_matrix(const void *d6, void *R, long long n) {
    ROT_FOR_EACH(i, n) {
        double a[6];
        Rot6d s;
        rot_load<T, 6>(d6, i, a);
        rot6d_fwd(a, s);
        rot_store<T, 9>(R, i, s.R);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_rot6d_to_matrix_bwd(const void *d6, const void *dR, void *dd6, long long n) {
    ROT_FOR_EACH(i, n) {
        double a[6], gR[9], ga[6];
        Rot6d s;
        rot_load<T, 6>(d6, i, a);
        rot_load<T, 9>(dR, i, gR);
        rot6d_fwd(a, s);
        rot6d_bwd(a, s, gR, ga);
        rot_store<T, 6>(dd6, i, ga);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_axis_angle_to_matrix(const void *aa, void *R, long long n) {
    ROT_FOR_EACH(i, n) {
        double a[3], r[9];
        RotAa s;
        rot_load<T, 3>(aa, i, a);
        rot_aa_fwd(a, s, r);
        rot_store<T, 9>(R, i, r);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_axis_angle_to_matrix_bwd(const void *aa, const void *dR, void *daa, long long n) {
    ROT_FOR_EACH(i, n) {
        double a[3], r[9], gR[9], ga[3];
        RotAa s;
        rot_load<T, 3>(aa, i, a);
        rot_load<T, 9>(dR, i, gR);
        rot_aa_fwd(a, s, r);
        rot_aa_bwd(a, s, gR, ga);
        rot_store<T, 3>(daa, i, ga);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_matrix_to_axis_angle(const void *R, void *aa, long long n) {
    ROT_FOR_EACH(i, n) {
        double m[9], a[3];
        RotMat s;
        rot_load<T, 9>(R, i, m);
        rot_mat_fwd(m, s, a);
        rot_store<T, 3>(aa, i, a);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_matrix_to_axis_angle_bwd(const void *R, const void *daa, void *dR, long long n) {
    ROT_FOR_EACH(i, n) {
        double m[9], a[3], ga[3], gm[9];
        RotMat s;
        rot_load<T, 9>(R, i, m);
        rot_load<T, 3>(daa, i, ga);
        rot_mat_fwd(m, s, a);
        rot_mat_bwd(s, ga, gm);
        rot_store<T, 9>(dR, i, gm);
    }
}

// 6-D -> axis-angle: the matrix lives in registers only
template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_rot6d_to_axis_angle(const void *d6, void *aa, long long n) {
    ROT_FOR_EACH(i, n) {
        double a[6], out[3];
        Rot6d s;
        RotMat q;
        rot_load<T, 6>(d6, i, a);
        rot6d_fwd(a, s);
        rot_mat_fwd(s.R, q, out);
        rot_store<T, 3>(aa, i, out);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_rot6d_distance(const void *p6, const void *t6, void *dist, long long n) {
    ROT_FOR_EACH(i, n) {
        double p[6], t[6], D[9];
        Rot6d sp, st;
        rot_load<T, 6>(p6, i, p);
        rot_load<T, 6>(t6, i, t);
        rot6d_fwd(p, sp);
        rot6d_fwd(t, st);
        const double d = rot_frobenius(sp.R, st.R, D);
        rot_store<T, 1>(dist, i, &d);
    }
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) k_rot6d_distance_bwd(const void *p6, const void *t6, const void *ddist, void *dp6, void *dt6,
                                                                      long long n) {
    ROT_FOR_EACH(i, n) {
        double p[6], t[6], D[9], up[1], g[6];
        Rot6d sp, st;
        rot_load<T, 6>(p6, i, p);
        rot_load<T, 6>(t6, i, t);
        rot_load<T, 1>(ddist, i, up);
        rot6d_fwd(p, sp);
        rot6d_fwd(t, st);
        const double d = rot_frobenius(sp.R, st.R, D);
        const double w = d > 0.0 ? up[0] / d : 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) D[k] *= w;
        if (dp6) {  // (wave-uniform)
            rot6d_bwd(p, sp, D, g);
            rot_store<T, 6>(dp6, i, g);
        }
        if (dt6) {
#pragma unroll
            for (int k = 0; k < 9; ++k) D[k] = -D[k];
            rot6d_bwd(t, st, D, g);
            rot_store<T, 6>(dt6, i, g);
        }
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------
static int rot_check(const char *who, int64_t n, int32_t dtype) {
    SMIL_REQUIRE(n >= 0, "%s: n=%lld must not be negative", who, (long long)n);
    SMIL_REQUIRE(dtype == SMIL_ROT_F32 || dtype == SMIL_ROT_F64, "%s: unknown dtype %d (SMIL_ROT_F32 or SMIL_ROT_F64)", who, dtype);
    return SMIL_OK;
}

// the checks every entry point shares, then the launch of kernel<float> or kernel<double> over n rotations (n == 0: nothing)
#define ROT_ENTRY(who, required, kernel, ...)                                                                            \
    do {                                                                                                                 \
        const int rc_ = rot_check(who, n, dtype);                                                                        \
        if (rc_ != SMIL_OK) return rc_;                                                                                  \
        if (n == 0) return SMIL_OK;                                                                                      \
        SMIL_REQUIRE(required, "%s: null argument", who);                                                                \
        const dim3 grid_((unsigned)std::min<long long>(ROT_MAX_BLOCKS, ((long long)n + ROT_THREADS - 1) / ROT_THREADS)); \
        if (dtype == SMIL_ROT_F32)                                                                                       \
            hipLaunchKernelGGL(kernel<float>, grid_, dim3(ROT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__, (long long)n); \
        else                                                                                                             \
            hipLaunchKernelGGL(kernel<double>, grid_, dim3(ROT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__, (long long)n); \
        SMIL_LAUNCH_CHECK();                                                                                             \
        return SMIL_OK;                                                                                                  \
    } while (0)

extern "C" int smil_rot6d_to_matrix(const void *d6, void *R, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_rot6d_to_matrix", d6 && R, k_rot6d_to_matrix, d6, R);
}
extern "C" int smil_rot6d_to_matrix_backward(const void *d6, const void *dR, void *dd6, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_rot6d_to_matrix_backward", d6 && dR && dd6, k_rot6d_to_matrix_bwd, d6, dR, dd6);
}
extern "C" int smil_axis_angle_to_matrix(const void *aa, void *R, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_axis_angle_to_matrix", aa && R, k_axis_angle_to_matrix, aa, R);
}
extern "C" int smil_axis_angle_to_matrix_backward(const void *aa, const void *dR, void *daa, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_axis_angle_to_matrix_backward", aa && dR && daa, k_axis_angle_to_matrix_bwd, aa, dR, daa);
}
extern "C" int smil_matrix_to_axis_angle(const void *R, void *aa, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_matrix_to_axis_angle", R && aa, k_matrix_to_axis_angle, R, aa);
}
extern "C" int smil_matrix_to_axis_angle_backward(const void *R, const void *daa, void *dR, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_matrix_to_axis_angle_backward", R && daa && dR, k_matrix_to_axis_angle_bwd, R, daa, dR);
}
extern "C" int smil_rot6d_to_axis_angle(const void *d6, void *aa, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_rot6d_to_axis_angle", d6 && aa, k_rot6d_to_axis_angle, d6, aa);
}
extern "C" int smil_rot6d_distance(const void *p6, const void *t6, void *dist, int64_t n, int32_t dtype, void *stream) {
    ROT_ENTRY("smil_rot6d_distance", p6 && t6 && dist, k_rot6d_distance, p6, t6, dist);
}
extern "C" int smil_rot6d_distance_backward(const void *p6, const void *t6, const void *ddist, void *dp6, void *dt6, int64_t n, int32_t dtype,
                                            void *stream) {
    ROT_ENTRY("smil_rot6d_distance_backward", p6 && t6 && ddist, k_rot6d_distance_bwd, p6, t6, ddist, dp6, dt6);
}
