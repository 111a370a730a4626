// Per-vertex arithmetic of linear blend skinning, forward and backward, shared by the separate kernels and the fused per-frame
// kernels of lbs.hip: both routes take every value below from the same expression.  The kernels keep their own loads, unroll
// structure and reductions; these helpers work on values that are already in registers or in LDS.
#pragma once
#include "common.h"

// One bone's term of the blended transform T = sum_k w_k A_k[:, :NC] (smal_torch.py:320-333): NC = 4, the 3x4 transform, row-major;
// NC = 3, its rotation part (3x3).  k: the bone's slot (0 .. SMIL_MAX_BONES - 1) in the vertex's packed ids, w its weight; sA: the
// frame's (J,12) transforms in LDS.  WIDE: the bone's three rows as three 16-byte LDS reads (sA 16-byte aligned; the fused
// kernels), else scalar reads of the entries that are used.  The caller zeroes T and walks the slots: the loop over the bones
// is part of each kernel's unroll structure.
template <int NC, bool WIDE>
__device__ __forceinline__ void blend_bone(float (&T)[3 * NC], const float *sA, uint32_t ids, int k, float w) {
    if (w == 0.f) return;
    const int bone = (ids >> (8 * k)) & 0xFF;
    if constexpr (WIDE) {
        const float4 *Ak = reinterpret_cast<const float4 *>(sA) + 3 * bone;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float4 r = Ak[m];
            T[NC * m] += w * r.x; T[NC * m + 1] += w * r.y; T[NC * m + 2] += w * r.z;
            if constexpr (NC == 4) T[NC * m + 3] += w * r.w;
        }
    } else {
        const float *Ak = sA + 12 * bone;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int c = 0; c < NC; ++c) T[NC * m + c] += w * Ak[4 * m + c];
    }
}

// o = T [x y z 1]^T: the skinned vertex before the frame's translation                              (smal_torch.py:335-340)
__device__ __forceinline__ void skin_point(const float (&T)[12], float x, float y, float z, float &ox, float &oy, float &oz) {
    ox = T[0] * x + T[1] * y + T[2] * z + T[3];
    oy = T[4] * x + T[5] * y + T[6] * z + T[7];
    oz = T[8] * x + T[9] * y + T[10] * z + T[11];
}

// o = T^T dv for the blended rotation T (3x3): the gradient on the vertex the transform was applied to (k_lbs_bwd_ndc writes this
// line out: see there)
__device__ __forceinline__ void skin_point_bwd(const float (&T)[9], const float (&dv)[3], float *o) {
#pragma unroll
    for (int n = 0; n < 3; ++n) o[n] = T[n] * dv[0] + T[3 + n] * dv[1] + T[6 + n] * dv[2];
}

// One entry of regressor^T d_joints, the gather over a vertex's column of the joint regressor (CSC): acc += w dj, for the entry's
// weight w and its joint's row dj of a (J,3) joint gradient
__device__ __forceinline__ void regressor_gather_term(float w, const float *dj, float (&acc)[3]) {
    acc[0] += w * dj[0]; acc[1] += w * dj[1]; acc[2] += w * dj[2];
}

// total upstream gradient on a posed vertex: d_verts + J_regressor (CSC gather) d_joints
__device__ __forceinline__ void vertex_upstream(const float *__restrict__ d_verts_b, const float *sDJ,
                                                const int *__restrict__ colptr, const int *__restrict__ row,
                                                const float *__restrict__ cval, int v, bool regress, float (&dv)[3]) {
    dv[0] = dv[1] = dv[2] = 0.f;
    if (d_verts_b) { dv[0] = d_verts_b[3 * v]; dv[1] = d_verts_b[3 * v + 1]; dv[2] = d_verts_b[3 * v + 2]; }
    if (regress)
        for (int e = colptr[v]; e < colptr[v + 1]; ++e) regressor_gather_term(cval[e], sDJ + 3 * row[e], dv);
}

// acc (3x4, a bone's d_A) += w dv (x) [x y z 1] for one vertex of the bone's list
__device__ __forceinline__ void bone_accumulate(float (&acc)[12], float w, const float *dv, float x, float y, float z) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float g = w * dv[r];
        acc[4 * r] += g * x; acc[4 * r + 1] += g * y; acc[4 * r + 2] += g * z; acc[4 * r + 3] += g;
    }
}

// One coordinate of one entry of a joint-regressor row (CSR): (p - t) w for the entry's weight w and its posed vertex's
// coordinate p.  t: the frame translation the vertices already carry when the reference regresses from the untranslated ones
// (fitter.py:280-281); the caller sums the row's entries over its lanes and adds t back.
__device__ __forceinline__ float regress_joint_term(float p, float t, float w) { return (p - t) * w; }
