// Steps of the kinematic chain of batch_global_rigid_transformation (reference smal_model/batch_lbs.py:31-50, 75-197) for float
// and double, in one order of operations.  Every function is one joint's share of one step, on registers (or LDS rows) the caller
// owns.  3x3 matrices are row-major (9), world transforms 3x4 row-major (12: [R | t] by rows).
//
// Users: joints.hip's float64 kernels take the Rodrigues pair and, in their forward walk, the chain_* steps.  lbs.hip's float32
// pose kernels (k_pose_fwd / k_chain_bwd) take the Rodrigues pair only: calling a chain_* step reschedules them, and lbs.hip is
// held to the code it emitted before.  The reverse steps of both files stay in their kernels: as functions they moved
// k_joints_bwd's bits or made its 2-D instantiations slower (profiles/chain_single_source.md has the figures).
//
//   local      L = diag(is) R diag(S)         is: 1 / scale of the parent (1 when scales propagate), S: own scale
//   root       G = [R | J]                    rotation only, own scale never applied (batch_lbs.py:151)
//   child      G = G_parent o [L | t]         t = J - J_parent (+ btrans, y flipped: batch_lbs.py:148 - at the call sites)
#pragma once
#include "common.h"

// batch_lbs.py:37-38: the norm is taken of theta + 1e-8, the axis uses the unshifted theta
template <class T>
__device__ __forceinline__ void rodrigues_fwd(const T th[3], T R[9]) {
    const T ax = th[0] + T(1e-8), ay = th[1] + T(1e-8), az = th[2] + T(1e-8);
    const T angle = sqrt(ax * ax + ay * ay + az * az);
    const T rx = th[0] / angle, ry = th[1] / angle, rz = th[2] / angle;
    const T c = cos(angle), s = sin(angle);
    const T k = T(1) - c;
    R[0] = c + k * rx * rx;      R[1] = k * rx * ry - s * rz; R[2] = k * rx * rz + s * ry;
    R[3] = k * ry * rx + s * rz; R[4] = c + k * ry * ry;      R[5] = k * ry * rz - s * rx;
    R[6] = k * rz * rx - s * ry; R[7] = k * rz * ry + s * rx; R[8] = c + k * rz * rz;
}

// dR (3x3) -> dtheta for R = c I + (1-c) r r^T + s H(r), angle = |theta + eps|, r = theta / angle
template <class T>
__device__ __forceinline__ void rodrigues_bwd(const T th[3], const T dR[9], T dth[3]) {
    const T ax = th[0] + T(1e-8), ay = th[1] + T(1e-8), az = th[2] + T(1e-8);
    const T angle = sqrt(ax * ax + ay * ay + az * az);
    const T inv = T(1) / angle;
    const T r[3] = {th[0] * inv, th[1] * inv, th[2] * inv};
    const T c = cos(angle), s = sin(angle), k = T(1) - c;
    // d angle through cos/sin:  sum dR_mn * (-s d_mn + s r_m r_n + c H_mn)
    const T trace = dR[0] + dR[4] + dR[8];
    T rdr = T(0);  // r^T dR r
    for (int m = 0; m < 3; ++m)
        for (int n = 0; n < 3; ++n) rdr += dR[3 * m + n] * r[m] * r[n];
    // sum dR_mn H_mn with H = [[0,-r2,r1],[r2,0,-r0],[-r1,r0,0]]
    const T hx = dR[7] - dR[5], hy = dR[2] - dR[6], hz = dR[3] - dR[1];
    const T dRH = r[0] * hx + r[1] * hy + r[2] * hz;
    T dangle = -s * trace + s * rdr + c * dRH;
    // d r_k = (1-c) ((dR + dR^T) r)_k + s * (hx,hy,hz)_k
    T dr[3];
    dr[0] = k * ((dR[0] + dR[0]) * r[0] + (dR[1] + dR[3]) * r[1] + (dR[2] + dR[6]) * r[2]) + s * hx;
    dr[1] = k * ((dR[3] + dR[1]) * r[0] + (dR[4] + dR[4]) * r[1] + (dR[5] + dR[7]) * r[2]) + s * hy;
    dr[2] = k * ((dR[6] + dR[2]) * r[0] + (dR[7] + dR[5]) * r[1] + (dR[8] + dR[8]) * r[2]) + s * hz;
    // r = theta / angle
    dangle -= (dr[0] * th[0] + dr[1] * th[1] + dr[2] * th[2]) * inv * inv;
    dth[0] = dr[0] * inv + dangle * ax * inv;
    dth[1] = dr[1] * inv + dangle * ay * inv;
    dth[2] = dr[2] * inv + dangle * az * inv;
}

// L = diag(is) R diag(S)
template <class T>
__device__ __forceinline__ void chain_local(const T is[3], const T R[9], const T S[3], T L[9]) {
    for (int m = 0; m < 3; ++m)
        for (int n = 0; n < 3; ++n) L[3 * m + n] = (is[m] * R[3 * m + n]) * S[n];
}

// the root's world transform: rotation only, own scale never applied (batch_lbs.py:151)
template <class T>
__device__ __forceinline__ void chain_root(const T R[9], const T J[3], T G[12]) {
    for (int m = 0; m < 3; ++m) {
        G[4 * m] = R[3 * m]; G[4 * m + 1] = R[3 * m + 1]; G[4 * m + 2] = R[3 * m + 2]; G[4 * m + 3] = J[m];
    }
}

// a child's world transform from its parent's P: G = P o [L | t]
template <class T>
__device__ __forceinline__ void chain_compose(const T *P, const T L[9], const T t[3], T G[12]) {
    for (int m = 0; m < 3; ++m) {
        const T p0 = P[4 * m], p1 = P[4 * m + 1], p2 = P[4 * m + 2], p3 = P[4 * m + 3];
        G[4 * m + 0] = p0 * L[0] + p1 * L[3] + p2 * L[6];
        G[4 * m + 1] = p0 * L[1] + p1 * L[4] + p2 * L[7];
        G[4 * m + 2] = p0 * L[2] + p1 * L[5] + p2 * L[8];
        G[4 * m + 3] = p0 * t[0] + p1 * t[1] + p2 * t[2] + p3;
    }
}
