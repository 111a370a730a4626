// Target image preparation for gfx950: the foreground bounds of silhouettes and ONE resampling kernel that undistorts, crops and
// resizes camera frames into the fitter's targets.
//
// Replaces (reference): cv2.undistort per frame (smal_fitter/sleap_data/preprocess_sleap_multiview_dataset.py:710-735, :969-1028) and
// crop_to_silhouette (smal_fitter/utils.py:7-49), host loops over single frames.  The semantics are stated at include/smilfit.h.
//
//  * k_image_bounds   exact integer reduction of one image (or one slab of rows of it): lanes stride over the pixels, wave minima /
//                     maxima / count by butterfly (common.h), the waves meet in LDS, one lane stores.  An image of more than BOUNDS_SPLIT
//                     pixels is cut into slabs whose results meet with integer atomics in a row that k_bounds_init has preset:
//                     minima, maxima and integer sums do not depend on the order, so the result is bit-reproducible either way.
//  * k_warp<T, C>     one output pixel (all C channels) per thread, consecutive threads on consecutive pixels of a row-major image:
//                     the stores are coalesced, the (at most four) taps are plain global loads, all issued before the first is
//                     used (a tap outside the image loads a stand-in pixel and is replaced by the border afterwards: a load under
//                     a per-lane condition would be a branch with a wait of its own).  The per-image tables are indexed
//                     by the workgroup's image alone, so they are scalar loads.  The coordinate arithmetic is float64 with
//                     contraction off - the map is specified to the bit (the nearest tap of a pixel must not depend on whether a
//                     compiler fused a multiply-add) - and the blend is three float32 lerps.  Nothing is staged in LDS: the taps
//                     of neighbouring pixels fall in the same or adjacent cache lines, and a lens moves them by a fraction of a
//                     pixel from one output pixel to the next.
#include <cmath>

#include "common.h"

#define BOUNDS_THREADS 256
#define BOUNDS_SPLIT (1 << 16)  // pixels of one workgroup (256 per thread)
#define BOUNDS_UNROLL 8         // pixels a thread has in flight
#define WARP_THREADS 256

// ---- bounds -----------------------------------------------------------------------------------------------------------------
__global__ void k_bounds_init(int *bounds, long long N, int H, int W) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int *b = bounds + 5 * (size_t)n;
    b[0] = H; b[1] = -1; b[2] = W; b[3] = -1; b[4] = 0;
}

template <typename T>
__global__ void __launch_bounds__(BOUNDS_THREADS) k_image_bounds(const T *sil, int H, int W, int slabs, int *bounds) {
    __shared__ int s_red[BOUNDS_THREADS / 64][5];
    const size_t n = blockIdx.x / (unsigned)slabs;
    const int slab = blockIdx.x % (unsigned)slabs;
    const int pixels = H * W;
    const int p0 = slab * BOUNDS_SPLIT, p1 = min(pixels, p0 + BOUNDS_SPLIT);  // (the host keeps H W <= 2^31 - 1 - 2^16, so p0 + BOUNDS_SPLIT fits an int)
    const T *img = sil + n * (size_t)pixels;
    int y_min = H, y_max = -1, x_min = W, x_max = -1, count = 0;
    // BOUNDS_UNROLL pixels per step, all loaded (the last one again where the slab ends) before any is looked at: one load and its
    // wait per pixel would leave every wave with a single byte in flight
    for (int p = p0 + (int)threadIdx.x; p < p1; p += BOUNDS_UNROLL * BOUNDS_THREADS) {
        T v[BOUNDS_UNROLL];
#pragma unroll
        for (int k = 0; k < BOUNDS_UNROLL; ++k) v[k] = img[min(p + k * BOUNDS_THREADS, p1 - 1)];
#pragma unroll
        for (int k = 0; k < BOUNDS_UNROLL; ++k) {
            const int q = p + k * BOUNDS_THREADS;
            if (q < p1 && v[k] > (T)0) {
                const int y = q / W, x = q - y * W;
                y_min = min(y_min, y); y_max = max(y_max, y);
                x_min = min(x_min, x); x_max = max(x_max, x);
                ++count;
            }
        }
    }
    y_min = wave_min(y_min); y_max = wave_max(y_max);
    x_min = wave_min(x_min); x_max = wave_max(x_max);
    count = wave_sum(count);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = y_min; s_red[wave][1] = y_max; s_red[wave][2] = x_min; s_red[wave][3] = x_max; s_red[wave][4] = count;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < BOUNDS_THREADS / 64; ++w) {
        y_min = min(y_min, s_red[w][0]); y_max = max(y_max, s_red[w][1]);
        x_min = min(x_min, s_red[w][2]); x_max = max(x_max, s_red[w][3]);
        count += s_red[w][4];
    }
    int *b = bounds + 5 * n;
    if (slabs == 1) {
        b[0] = y_min; b[1] = y_max; b[2] = x_min; b[3] = x_max; b[4] = count;
    } else if (count > 0) {  // (an empty slab leaves the preset row as it is)
        atomicMin(b + 0, y_min); atomicMax(b + 1, y_max);
        atomicMin(b + 2, x_min); atomicMax(b + 3, x_max);
        atomicAdd(b + 4, count);
    }
}

extern "C" int smil_image_bounds(const void *sil, int32_t sil_is_u8, int64_t N, int32_t H, int32_t W, int32_t *bounds, void *stream_) {
    SMIL_REQUIRE(N >= 0 && H > 0 && W > 0, "smil_image_bounds: bad sizes N=%lld H=%d W=%d", (long long)N, H, W);
    SMIL_REQUIRE((int64_t)H * W <= 0x7FFFFFFF - BOUNDS_SPLIT, "smil_image_bounds: H W = %d x %d pixels exceed a 32-bit pixel index", H, W);
    const int64_t slabs = ((int64_t)H * W + BOUNDS_SPLIT - 1) / BOUNDS_SPLIT;
    SMIL_REQUIRE(N * slabs <= 0x7FFFFFFF, "smil_image_bounds: N = %lld images of %lld slabs exceed the grid", (long long)N, (long long)slabs);
    if (N == 0) return SMIL_OK;
    SMIL_REQUIRE(sil && bounds, "smil_image_bounds: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    if (slabs > 1) {
        hipLaunchKernelGGL(k_bounds_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (int *)bounds, (long long)N, H, W);
        SMIL_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)(N * slabs));
    if (sil_is_u8)
        hipLaunchKernelGGL(k_image_bounds<unsigned char>, grid, dim3(BOUNDS_THREADS), 0, stream, (const unsigned char *)sil, H, W, (int)slabs,
                           (int *)bounds);
    else
        hipLaunchKernelGGL(k_image_bounds<float>, grid, dim3(BOUNDS_THREADS), 0, stream, (const float *)sil, H, W, (int)slabs, (int *)bounds);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---- the warp ---------------------------------------------------------------------------------------------------------------
#define WARP_COORD_LIMIT 1073741824.0  // 2^30: a finite coordinate beyond it is moved here, where every tap is still outside any image

struct WarpArgs {
    const void *src;
    void *out;
    const double *affine, *K, *K_new, *dist;
    const int *clamp;
    const float *border;
    int N_src, H, W, S_h, S_w, chunks;
    int n_affine, n_lens, n_clamp, n_border;
    int coord_mode, interp, planar, out_is_u8;
    float scale;
};

// cv2.undistort's map (initUndistortRectifyMap as documented, five coefficients): the pixel (u, v) of the camera K_new shows the
// pixel of the distorted camera K that is returned in (u, v).  Evaluated as written at include/smilfit.h, powers by repeated products.
__device__ __forceinline__ void distort5(const double *K, const double *Kn, const double *d, double &u, double &v) {
#pragma clang fp contract(off)
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    const double x = (u - Kn[2]) / Kn[0], y = (v - Kn[5]) / Kn[4];
    const double r2 = x * x + y * y;
    const double radial = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2);
    const double xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x));
    const double yd = y * radial + p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y;
    u = K[0] * xd + K[2];
    v = K[4] * yd + K[5];
}

// One axis of an output pixel: its first tap and the fraction towards the next (0 for nearest).  ok: the coordinate was finite.
struct AxisTap { int t; float w; bool ok; };
__device__ __forceinline__ AxisTap exact_tap(double u, int interp) {
#pragma clang fp contract(off)
    AxisTap a;
    a.ok = u - u == 0.0;  // finite
    u = fmin(fmax(a.ok ? u : 0.0, -WARP_COORD_LIMIT), WARP_COORD_LIMIT);
    if (interp == SMIL_WARP_BILINEAR) {
        const double f = floor(u);
        a.t = (int)f;
        a.w = (float)(u - f);
    } else {
        a.t = (int)floor(u + 0.5);
        a.w = 0.f;
    }
    return a;
}
__device__ __forceinline__ AxisTap resize_tap(int j, double a_, double b_, int mode) {
#pragma clang fp contract(off)
    AxisTap a;
    a.ok = true;
    const double origin = fmin(fmax(b_ == b_ ? b_ : 0.0, -WARP_COORD_LIMIT), WARP_COORD_LIMIT);  // (integral by specification)
    if (mode == SMIL_WARP_RESIZE_LINEAR) {
        float f = (float)(((double)j + 0.5) * a_ - 0.5);
        f = fminf(fmaxf(f == f ? f : 0.f, -(float)WARP_COORD_LIMIT), (float)WARP_COORD_LIMIT);
        const float fl = floorf(f);
        a.t = (int)fmin(fmax(origin + (double)fl, -WARP_COORD_LIMIT), WARP_COORD_LIMIT);
        a.w = f - fl;
    } else {
        double f = floor((double)j * a_);
        f = fmin(fmax(f == f ? f : 0.0, -WARP_COORD_LIMIT), WARP_COORD_LIMIT);
        a.t = (int)fmin(fmax(origin + f, -WARP_COORD_LIMIT), WARP_COORD_LIMIT);
        a.w = 0.f;
    }
    return a;
}

__device__ __forceinline__ float lerp_once(float a, float b, float w) {
#pragma clang fp contract(off)
    return a + w * (b - a);
}

template <typename T, int C>
__global__ void __launch_bounds__(WARP_THREADS) k_warp(WarpArgs a) {
    const size_t n = blockIdx.x / (unsigned)a.chunks;  // (wave-uniform: the tables below are scalar loads)
    const int p = (int)(blockIdx.x % (unsigned)a.chunks) * WARP_THREADS + (int)threadIdx.x;
    if (p >= a.S_h * a.S_w) return;
    const int i = p / a.S_w, j = p - i * a.S_w;

    const double *af = a.affine + 4 * (n % (unsigned)a.n_affine);
    AxisTap tx, ty;
    if (a.coord_mode == SMIL_WARP_EXACT) {
        double u, v;
        {
#pragma clang fp contract(off)
            u = af[0] * (double)j + af[1];
            v = af[2] * (double)i + af[3];
        }
        if (a.K) {
            const size_t l = n % (unsigned)a.n_lens;
            distort5(a.K + 9 * l, a.K_new + 9 * l, a.dist + 5 * l, u, v);
        }
        tx = exact_tap(u, a.interp);
        ty = exact_tap(v, a.interp);
    } else {
        tx = resize_tap(j, af[0], af[1], a.coord_mode);
        ty = resize_tap(i, af[2], af[3], a.coord_mode);
    }
    const bool two = a.interp == SMIL_WARP_BILINEAR;
    int x0 = tx.t, x1 = tx.t + 1, y0 = ty.t, y1 = ty.t + 1;
    if (a.clamp) {
        const int *r = a.clamp + 4 * (n % (unsigned)a.n_clamp);
        x0 = min(max(x0, r[0]), r[1]); x1 = min(max(x1, r[0]), r[1]);
        y0 = min(max(y0, r[2]), r[3]); y1 = min(max(y1, r[2]), r[3]);
    }
    const bool finite = tx.ok && ty.ok;
    const bool in_x0 = finite && x0 >= 0 && x0 < a.W, in_x1 = finite && x1 >= 0 && x1 < a.W;
    const bool in_y0 = y0 >= 0 && y0 < a.H, in_y1 = y1 >= 0 && y1 < a.H;

    const T *img = (const T *)a.src + (n % (unsigned)a.N_src) * ((size_t)a.H * a.W * C);
    const float *border = a.border + C * (n % (unsigned)a.n_border);
    const size_t r0 = (size_t)(in_y0 ? y0 : 0) * a.W, r1 = (size_t)(in_y1 ? y1 : 0) * a.W;  // (a tap outside the image: row / column 0 stands in)
    const size_t c0 = in_x0 ? x0 : 0, c1 = in_x1 ? x1 : 0;
    // Every tap is LOADED, from its own pixel or from the stand-in pixel above, and the border is selected afterwards: a load under
    // a per-lane condition is a branch with its own wait, and twelve of them in a row are twelve memory latencies per wave.
    const T *pa = img + (r0 + c0) * C, *pb = img + (r0 + c1) * C, *pc = img + (r1 + c0) * C, *pd = img + (r1 + c1) * C;
    const bool in_a = in_x0 && in_y0, in_b = in_x1 && in_y0, in_c = in_x0 && in_y1, in_d = in_x1 && in_y1;
    float val[C];
    if (two) {
        T la[C], lb[C], lc[C], ld[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            la[c] = pa[c]; lb[c] = pb[c]; lc[c] = pc[c]; ld[c] = pd[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float bc = border[c];
            const float ta = in_a ? (float)la[c] : bc, tb = in_b ? (float)lb[c] : bc, tc = in_c ? (float)lc[c] : bc, td = in_d ? (float)ld[c] : bc;
            const float top = lerp_once(ta, tb, tx.w), bottom = lerp_once(tc, td, tx.w);
            val[c] = lerp_once(top, bottom, ty.w) * a.scale;
        }
    } else {
        T la[C];
#pragma unroll
        for (int c = 0; c < C; ++c) la[c] = pa[c];
#pragma unroll
        for (int c = 0; c < C; ++c) val[c] = (in_a ? (float)la[c] : border[c]) * a.scale;
    }
    const size_t plane = (size_t)a.S_h * a.S_w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const size_t o = a.planar ? (n * C + c) * plane + p : (n * plane + p) * C + c;
        if (a.out_is_u8) ((unsigned char *)a.out)[o] = (unsigned char)rintf(fminf(fmaxf(val[c], 0.f), 255.f));  // (a NaN becomes 0)
        else ((float *)a.out)[o] = val[c];
    }
}

template <typename T>
static void launch_warp(const WarpArgs &a, int C, dim3 grid, hipStream_t stream) {
    switch (C) {
    case 1: hipLaunchKernelGGL((k_warp<T, 1>), grid, dim3(WARP_THREADS), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((k_warp<T, 2>), grid, dim3(WARP_THREADS), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_warp<T, 3>), grid, dim3(WARP_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL((k_warp<T, 4>), grid, dim3(WARP_THREADS), 0, stream, a); break;
    }
}

extern "C" int smil_warp_images(const SmilWarp *w, void *stream_) {
    SMIL_REQUIRE(w, "smil_warp_images: null argument");
    SMIL_REQUIRE(w->N >= 0 && w->N_src > 0 && w->H > 0 && w->W > 0 && w->S_h > 0 && w->S_w > 0,
                 "smil_warp_images: bad sizes N=%d N_src=%d H=%d W=%d S_h=%d S_w=%d", w->N, w->N_src, w->H, w->W, w->S_h, w->S_w);
    SMIL_REQUIRE(w->C >= 1 && w->C <= 4, "smil_warp_images: C=%d must be 1 .. 4", w->C);
    SMIL_REQUIRE(w->coord_mode >= SMIL_WARP_EXACT && w->coord_mode <= SMIL_WARP_RESIZE_NEAREST, "smil_warp_images: unknown coordinate mode %d",
                 w->coord_mode);
    SMIL_REQUIRE(w->interp == SMIL_WARP_NEAREST || w->interp == SMIL_WARP_BILINEAR, "smil_warp_images: unknown interpolation %d", w->interp);
    SMIL_REQUIRE(w->coord_mode == SMIL_WARP_EXACT || w->interp == (w->coord_mode == SMIL_WARP_RESIZE_LINEAR ? SMIL_WARP_BILINEAR : SMIL_WARP_NEAREST),
                 "smil_warp_images: coordinate mode %d has its own interpolation, not %d", w->coord_mode, w->interp);
    const bool lens = w->K || w->K_new || w->dist;
    SMIL_REQUIRE(!lens || (w->K && w->K_new && w->dist), "smil_warp_images: K, K_new and dist come together");
    SMIL_REQUIRE(!lens || w->coord_mode == SMIL_WARP_EXACT, "smil_warp_images: a lens needs the exact coordinate mode");
    SMIL_REQUIRE(w->n_affine >= 1 && w->n_border >= 1 && (!lens || w->n_lens >= 1) && (!w->clamp || w->n_clamp >= 1),
                 "smil_warp_images: a table needs at least one row (affine %d, border %d, lens %d, clamp %d)", w->n_affine, w->n_border,
                 w->n_lens, w->n_clamp);
    // what a thread indexes: a pixel of an output image and the taps of a row as int, the image's chunks times N as the grid
    SMIL_REQUIRE(w->H < (1 << 30) && w->W < (1 << 30), "smil_warp_images: H=%d W=%d must stay below 2^30", w->H, w->W);
    SMIL_REQUIRE((int64_t)w->S_h * w->S_w <= 0x7FFFFFFF - WARP_THREADS, "smil_warp_images: S_h S_w = %d x %d pixels exceed a 32-bit pixel index",
                 w->S_h, w->S_w);
    const int64_t chunks = ((int64_t)w->S_h * w->S_w + WARP_THREADS - 1) / WARP_THREADS;
    SMIL_REQUIRE(chunks * w->N <= 0x7FFFFFFF, "smil_warp_images: N = %d images of %lld workgroups exceed the grid", w->N, (long long)chunks);
    if (w->N == 0) return SMIL_OK;
    SMIL_REQUIRE(w->src && w->out && w->affine && w->border, "smil_warp_images: null argument");
    WarpArgs a;
    a.src = w->src; a.out = w->out; a.affine = w->affine; a.K = w->K; a.K_new = w->K_new; a.dist = w->dist;
    a.clamp = (const int *)w->clamp; a.border = w->border;
    a.N_src = w->N_src; a.H = w->H; a.W = w->W; a.S_h = w->S_h; a.S_w = w->S_w; a.chunks = (int)chunks;
    a.n_affine = w->n_affine; a.n_lens = lens ? w->n_lens : 1; a.n_clamp = w->clamp ? w->n_clamp : 1; a.n_border = w->n_border;
    a.coord_mode = w->coord_mode; a.interp = w->interp; a.planar = w->planar != 0; a.out_is_u8 = w->out_is_u8 != 0;
    a.scale = w->scale;
    const dim3 grid((unsigned)(chunks * w->N));
    if (w->src_is_u8) launch_warp<unsigned char>(a, w->C, grid, (hipStream_t)stream_);
    else launch_warp<float>(a, w->C, grid, (hipStream_t)stream_);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
