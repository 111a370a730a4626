// FoV-perspective camera of one image: world -> view -> NDC -> screen, forward and backward, for project.hip and the fused
// per-frame kernels of lbs.hip.  Arithmetic restated from pytorch3d 0.7.x (see project.hip).  Included by common.h.
//
// A camera set may carry a principal point (SmilCameras.principal: pytorch3d's PerspectiveCameras in NDC,
// x_ndc = K00 x / z + px).  load_camera and camera_project take it as a template parameter PP: k_project (project.hip) is instantiated
// twice and the host picks by cam->principal != NULL, so the centred instantiation holds the instructions it held before the table
// existed (the suite pins its last bits).  The fused per-frame forward (lbs.hip) runs centred cameras only: with a table
// smil_lbs_forward_project takes the separate kernels and k_project<true>, whose bits it is specified to return.  The backward helpers take no such parameter: they recompute the UNSHIFTED x_ndc = vx k00 / z from
// the world point, which is what d z_view and the fov sum need - px depends on neither the point nor the fov.
#pragma once
#include <hip/hip_runtime.h>

#include "smilfit.h"

#define SMIL_ZNEAR 0.001f  // Renderer.DEFAULT_ZNEAR (p3d_renderer.py:24)

// Sixteen floats: also a row of the (views,16) array a workgroup stages its frame's cameras in (LDS).
struct CamParams {
    float R[9];
    float T[3];
    float k00, k11;
    float px, py;  // principal point (NDC); written and read by the PP instantiations only
};
static_assert(sizeof(CamParams) == 16 * sizeof(float), "a staged camera is sixteen floats");

template <bool PP = false>
__device__ __forceinline__ CamParams load_camera(const SmilCameras &c, int n) {
    CamParams p;
    const float *R = c.R + (size_t)(n % c.nR) * 9;
    const float *T = c.T + (size_t)(n % c.nT) * 3;
    for (int i = 0; i < 9; ++i) p.R[i] = R[i];
    for (int i = 0; i < 3; ++i) p.T[i] = T[i];
    const float fov = c.fov[n % c.nFov];
    const float asp = c.aspect ? c.aspect[n % c.nAspect] : 1.0f;
    const float t = tanf((fov * 0.017453292519943295f) / 2.0f);
    const float max_y = t * SMIL_ZNEAR;
    const float max_x = max_y * asp;
    p.k00 = 2.0f * SMIL_ZNEAR / (max_x - (-max_x));
    p.k11 = 2.0f * SMIL_ZNEAR / (max_y - (-max_y));
    if (PP) {
        const float *pp = c.principal + (size_t)(n % c.nPrincipal) * 2;
        p.px = pp[0]; p.py = pp[1];
    }
    return p;
}

// A workgroup stages its frame's cameras in LDS as a (views,16) float array: row `view` of it as a camera ...
__device__ __forceinline__ CamParams &staged_camera(float *sCam, int view) { return *reinterpret_cast<CamParams *>(sCam + 16 * view); }
// ... and image n's camera written to a row: what the staged projections read (R, T, k00, k11: the fused kernels run centred cameras
// forward, and backward no principal point enters)
__device__ __forceinline__ void stage_camera(CamParams &row, const SmilCameras &c, int n) {
    const CamParams cp = load_camera(c, n);
    for (int i = 0; i < 9; ++i) row.R[i] = cp.R[i];
    for (int i = 0; i < 3; ++i) row.T[i] = cp.T[i];
    row.k00 = cp.k00; row.k11 = cp.k11;
}

// world point -> (x_ndc, y_ndc, z_view).  PP: the principal point is added AFTER the division (a quotient is no product: nothing
// contracts with the add, and the shifted value is the centred one plus one rounding)
template <bool PP = false>
__device__ __forceinline__ void camera_project(const CamParams &cp, float x, float y, float z, float &xn, float &yn, float &vz) {
    const float vx = x * cp.R[0] + y * cp.R[3] + z * cp.R[6] + cp.T[0];
    const float vy = x * cp.R[1] + y * cp.R[4] + z * cp.R[7] + cp.T[1];
    const float vz_ = x * cp.R[2] + y * cp.R[5] + z * cp.R[8] + cp.T[2];
    xn = vx * cp.k00 / vz_;
    yn = vy * cp.k11 / vz_;
    if (PP) { xn += cp.px; yn += cp.py; }
    vz = vz_;
}

// NDC -> screen for an S x S image, hS = S / 2, in the reference's (y, x) order
__device__ __forceinline__ void ndc_to_yx(float hS, float xn, float yn, float *yx) {
    yx[0] = hS - hS * yn;
    yx[1] = hS - hS * xn;
}

// Gradient (dxn, dyn) on a point's NDC position added to the gradient (gx, gy, gz) on the world point.  Returns the point's
// share of the image's raw fov sum (x_ndc, y_ndc ~ 1 / tan(fov/2): smil_fov_reduce).  xn, yn below are the UNSHIFTED coordinates
// whether or not the cameras carry a principal point (see the head of this file).  The fused LBS backward calls this for joints
// and vertices; k_project_bwd (project.hip) keeps these lines and those of unpack_d_ndc in its own order, for the sake of its last bit.
__device__ __forceinline__ float camera_project_bwd(const CamParams &cp, float x, float y, float z, float dxn, float dyn, float &gx,
                                                    float &gy, float &gz) {
    const float vx = x * cp.R[0] + y * cp.R[3] + z * cp.R[6] + cp.T[0];
    const float vy = x * cp.R[1] + y * cp.R[4] + z * cp.R[7] + cp.T[1];
    const float vz = x * cp.R[2] + y * cp.R[5] + z * cp.R[8] + cp.T[2];
    const float iz = 1.0f / vz;
    const float xn = vx * cp.k00 * iz, yn = vy * cp.k11 * iz;
    const float dvx = dxn * cp.k00 * iz, dvy = dyn * cp.k11 * iz;
    const float dvz = -(xn * dxn + yn * dyn) * iz;
    gx += cp.R[0] * dvx + cp.R[1] * dvy + cp.R[2] * dvz;
    gy += cp.R[3] * dvx + cp.R[4] * dvy + cp.R[5] * dvz;
    gz += cp.R[6] * dvx + cp.R[7] * dvy + cp.R[8] * dvz;
    return dxn * xn + dyn * yn;
}

// One point's row of d_ndc (N,P,2) of an image whose factor `scale` is not 0 (0: the row is two plain floats, and the caller
// takes them as they are): what the fused rasteriser left (the encoder: `pack_fx2`, raster_common.h), x and y as two 32-bit
// fixed-point numbers in one 64-bit word, x * 2^32 + y in two's complement - a negative y borrowed one from the high word - times
// `scale`; under a negative factor the row reads as zero.
__device__ __forceinline__ void unpack_d_ndc(const float2 &raw, float scale, float &dxn, float &dyn) {
    const int qy = __float_as_int(raw.x), qx = __float_as_int(raw.y) - (qy >> 31);
    dxn = scale > 0.f ? (float)qx * scale : 0.f;
    dyn = scale > 0.f ? (float)qy * scale : 0.f;
}

// Depth gradient dz of a cut edge's end point (SmilClipDepth) added to the world-space gradient dv[3] of its vertex:
// z_view = x R[2] + y R[5] + z R[8] + T_z.  Several images or entries may meet in one vertex: float atomics.
__device__ __forceinline__ void clip_depth_bwd(const CamParams &cp, float dz, float *dv) {
    atomicAdd(dv, dz * cp.R[2]); atomicAdd(dv + 1, dz * cp.R[5]); atomicAdd(dv + 2, dz * cp.R[8]);
}
