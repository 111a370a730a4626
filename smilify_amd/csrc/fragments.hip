// Fragments of the hard rasteriser and the keypoint self-occlusion test against a depth buffer, for gfx950.
//
// Replaces (reference): what pytorch3d's MeshRasterizer(blur_radius=0, faces_per_pixel=1, bin_size=0) of smal_fitter/p3d_renderer.py:54-70
// returns as Fragments (pix_to_face, zbuf, bary_coords; un-vendored, restated as in shade.hip), and
// smal_fitter/Unreal2Pytorch3D.py:664-760 refine_visibility_with_depth (called per view at :1558-1580), for all images of a batch.
//
//  * k_fragment_background  the wanted outputs as background: pix_to_face -1, zbuf -1, bary -1, dist +inf.
//  * k_fragment_tiles       the tile sweep of the colour kernel (raster_hard.h) with an epilogue that writes the winner instead of
//                           shading it: original face id, its view depth, its barycentrics with respect to the original face, and the
//                           Euclidean distance |C - X| from the camera centre C = -T R^T to the world point X = sum b_c verts_world[P_c],
//                           both formed as the colour epilogue forms them.  Every output is optional (wave-uniform branches on the
//                           pointers); nothing that only `dist` needs is loaded without it.  No vertex normals, no atomics: two calls are
//                           bit-identical.
//  * k_depth_visibility     thread per (image, keypoint): the minimum of the depth buffer over the keypoint's window against the
//                           keypoint's own distance to the camera, in float64 throughout.
#include <algorithm>

#include "common.h"
#include "raster_hard.h"

#define FRAGMENT_WAVES_PER_CU 28  // single-wave workgroups per CU of the tile kernel's grid, as the colour kernel's
#define VIS_MAX_HALF_WINDOW 8

// ---------------------------------------------------------------------------------------------
// fragments
// ---------------------------------------------------------------------------------------------
struct FragmentArgs {
    ColourSetup cs;
    const float *verts_ndc;    // (N,V,3)
    const float *verts_world;  // (frames,V,3) or NULL without dist
    const int *faces;          // (F,3)
    SmilCameras cam;
    int *pix_to_face;          // (N,S,S) or NULL
    float *zbuf;               // (N,S,S) or NULL
    float *bary;               // (N,S,S,3) or NULL
    float *dist;               // (N,S,S) or NULL
    int N, V, F, S, tiles_x, views;
    float z_clip;
};

__global__ void __launch_bounds__(256) k_fragment_background(int *__restrict__ p2f, float *__restrict__ zbuf, float *__restrict__ bary,
                                                             float *__restrict__ dist, size_t n_pix) {
    // (plain 4-byte stores: a slice of a batch need not start on a 16-byte boundary)
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p2f)
        for (size_t i = first; i < n_pix; i += stride) p2f[i] = -1;
    if (zbuf)
        for (size_t i = first; i < n_pix; i += stride) zbuf[i] = -1.0f;
    if (bary)
        for (size_t i = first; i < 3 * n_pix; i += stride) bary[i] = -1.0f;
    if (dist)
        for (size_t i = first; i < n_pix; i += stride) dist[i] = __builtin_inff();
}

__global__ void __launch_bounds__(64) k_fragment_tiles(FragmentArgs a) {
    const int S = a.S, V = a.V;
    hard_tile_sweep(a, [&](int img, size_t pix, int orig, int P0, int P1, int P2, const float (&b)[3], float pz) {
        const size_t o = (size_t)img * S * S + pix;
        if (a.pix_to_face) a.pix_to_face[o] = orig;
        if (a.zbuf) a.zbuf[o] = pz;
        if (a.bary) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.bary[3 * o + c] = b[c];
        }
        if (a.dist) {
            const int frame = img / a.views;
            const float *Xw = a.verts_world + (size_t)frame * V * 3;
            const int Pi[3] = {P0, P1, P2};
            float X[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int q = 0; q < 3; ++q) X[q] = fmaf(b[c], Xw[3 * Pi[c] + q], X[q]);
            // camera centre C = -T R^T (X_view = X_world R + T)
            const float *R = a.cam.R + (size_t)(img % a.cam.nR) * 9;
            const float *T = a.cam.T + (size_t)(img % a.cam.nT) * 3;
            float C[3], v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) C[q] = -(T[0] * R[3 * q] + T[1] * R[3 * q + 1] + T[2] * R[3 * q + 2]);
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = C[q] - X[q];
            a.dist[o] = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
    });
}

extern "C" size_t smil_fragments_workspace_bytes(const SmilModel *m, int32_t N, int32_t S) {
    return (m && N > 0 && S > 0) ? smil_colour_setup_bytes(m, N, S) : 0;
}

extern "C" int smil_render_fragments(const SmilModel *m, const SmilCameras *cam, const float *verts_world, const float *verts_ndc,
                                     int32_t *pix_to_face, float *zbuf, float *bary, float *dist, void *workspace, void *stream_) {
    SMIL_REQUIRE(m && cam && verts_ndc && workspace, "smil_render_fragments: null argument");
    SMIL_REQUIRE(pix_to_face || zbuf || bary || dist, "smil_render_fragments: no output asked for");
    SMIL_REQUIRE(cam->N > 0 && cam->views > 0 && cam->N % cam->views == 0 && cam->S > 0, "smil_render_fragments: bad sizes N=%d views=%d S=%d",
                 cam->N, cam->views, cam->S);
    if (dist) {
        SMIL_REQUIRE(verts_world, "smil_render_fragments: dist needs verts_world");
        SMIL_REQUIRE(cam->R && cam->T && cam->nR > 0 && cam->nT > 0, "smil_render_fragments: camera tables missing");
        for (int k : {cam->nR, cam->nT})
            SMIL_REQUIRE(k == 1 || k == cam->views || k == cam->N, "smil_render_fragments: camera table of %d rows for %d images, %d views", k,
                         cam->N, cam->views);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int N = cam->N, S = cam->S;
    FragmentArgs a;
    int rc = smil_colour_setup(m, verts_ndc, N, S, 0.5f * SMIL_ZNEAR, workspace, stream, &a.cs);
    if (rc) return rc;
    {
        const size_t n_pix = (size_t)N * S * S;
        const unsigned int grid = (unsigned int)std::min<size_t>((n_pix + 255) / 256, (size_t)256 * 64);
        hipLaunchKernelGGL(k_fragment_background, dim3(grid), dim3(256), 0, stream, (int *)pix_to_face, zbuf, bary, dist, n_pix);
        SMIL_LAUNCH_CHECK();
    }
    a.verts_ndc = verts_ndc; a.verts_world = verts_world; a.faces = m->faces; a.cam = *cam;
    a.pix_to_face = pix_to_face; a.zbuf = zbuf; a.bary = bary; a.dist = dist;
    a.N = N; a.V = m->V; a.F = m->F; a.S = S; a.tiles_x = ceil_div(S, TILE); a.views = cam->views; a.z_clip = 0.5f * SMIL_ZNEAR;
    hipLaunchKernelGGL(k_fragment_tiles, dim3((unsigned int)smil_device_limits().cus * FRAGMENT_WAVES_PER_CU), dim3(64), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---------------------------------------------------------------------------------------------
// depth visibility
// ---------------------------------------------------------------------------------------------
struct VisibilityArgs {
    const void *depth;      // u8 (B,H,W,C), depth in channel 0, or float (B,H,W) distances (+inf: background)
    const double *kp_norm;  // (B,P,2) (norm_x: along the rows, norm_y: along the columns)
    const double *kp_dist;  // (B,P)
    const float *vis_in;    // (B,P)
    float *vis_out;         // (B,P)
    double *surface;        // (B,P) or NULL
    double depth_max, tolerance;
    long long n;            // B * P
    int H, W, C, P, h;
};

template <bool U8>
__global__ void __launch_bounds__(256) k_depth_visibility(VisibilityArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float vis = a.vis_in[i];
    const double d = a.kp_dist[i];
    const double nx = a.kp_norm[2 * i], ny = a.kp_norm[2 * i + 1];
    double surface = __builtin_nan("");
    float out = vis;
    // (a NaN coordinate fails the range test; a non-finite distance is a keypoint without a 3-D position)
    if (vis != 0.0f && isfinite(d) && nx >= 0.0 && nx <= 1.0 && ny >= 0.0 && ny <= 1.0) {
        const int H = a.H, W = a.W;
        const int row = min(max((int)(nx * (double)H), 0), H - 1), col = min(max((int)(ny * (double)W), 0), W - 1);
        const int r0 = max(0, row - a.h), r1 = min(H, row + a.h + 1), c0 = max(0, col - a.h), c1 = min(W, col + a.h + 1);
        const size_t img = (size_t)(i / a.P) * H * W;
        if (U8) {
            const unsigned char *D = (const unsigned char *)a.depth;
            int m = 255;  // (the minimum on the bytes, before the conversion)
            for (int r = r0; r < r1; ++r)
                for (int c = c0; c < c1; ++c) m = min(m, (int)D[(img + (size_t)r * W + c) * a.C]);
            surface = ((double)m / 255.0) * a.depth_max;
        } else {
            const float *D = (const float *)a.depth;
            float m = __builtin_inff();
            for (int r = r0; r < r1; ++r)
                for (int c = c0; c < c1; ++c) m = fminf(m, D[img + (size_t)r * W + c]);
            surface = (double)m;
        }
        if (d > surface + a.tolerance) out = 0.0f;
    }
    a.vis_out[i] = out;
    if (a.surface) a.surface[i] = surface;
}

extern "C" int smil_depth_visibility(const void *depth, int32_t depth_is_u8, int32_t channels, double depth_max, int32_t B, int32_t H, int32_t W,
                                     const double *kp_norm, const double *kp_dist, int32_t P, const float *vis_in, double tolerance,
                                     int32_t neighborhood, float *vis_out, double *surface, void *stream_) {
    SMIL_REQUIRE(B >= 0 && P >= 0 && H > 0 && W > 0, "smil_depth_visibility: bad sizes B=%d P=%d H=%d W=%d", B, P, H, W);
    SMIL_REQUIRE(neighborhood >= 0 && neighborhood <= VIS_MAX_HALF_WINDOW, "smil_depth_visibility: neighborhood=%d outside [0, %d]", neighborhood,
                 VIS_MAX_HALF_WINDOW);
    SMIL_REQUIRE(!depth_is_u8 || channels >= 1, "smil_depth_visibility: channels=%d", channels);
    SMIL_REQUIRE(!depth_is_u8 || (depth_max == depth_max), "smil_depth_visibility: depth_max is NaN");
    if ((long long)B * P == 0) return SMIL_OK;
    SMIL_REQUIRE(depth && kp_norm && kp_dist && vis_in && vis_out, "smil_depth_visibility: null argument");
    VisibilityArgs a;
    a.depth = depth; a.kp_norm = kp_norm; a.kp_dist = kp_dist; a.vis_in = vis_in; a.vis_out = vis_out; a.surface = surface;
    a.depth_max = depth_max; a.tolerance = tolerance;
    a.n = (long long)B * P; a.H = H; a.W = W; a.C = depth_is_u8 ? channels : 1; a.P = P; a.h = neighborhood;
    const long long blocks = (a.n + 255) / 256;
    SMIL_REQUIRE(blocks <= 0x7FFFFFFFll, "smil_depth_visibility: B P = %lld keypoints exceed the grid", a.n);
    hipStream_t stream = (hipStream_t)stream_;
    if (depth_is_u8) hipLaunchKernelGGL(k_depth_visibility<true>, dim3((unsigned int)blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_depth_visibility<false>, dim3((unsigned int)blocks), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
