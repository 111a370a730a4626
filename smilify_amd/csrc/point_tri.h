// The closest point of a closed triangle to a point, once for float (the search) and once for double (the finish): point_mesh.hip.
//
// The seven Voronoi regions of a triangle a, b, c (Ericson, Real-Time Collision Detection, section 5.1.5, written from the book's
// description): with e1 = b - a, e2 = c - a and the six products d1 = e1.ap, d2 = e2.ap, d3 = e1.bp, d4 = e2.bp, d5 = e1.cp, d6 = e2.cp
// the regions are tried in the order A, B, edge AB, C, edge AC, edge BC, interior, and the first that holds decides.  Written as
// selects applied in the reverse order, so that every lane of a wave runs the same instructions.
//
// Degenerate triangles need no case of their own, with two additions to the book's tests:
//  * an edge region also asks that its denominator is > 0.  It is a sum of two non-negative terms that equals the edge's squared length
//    in exact arithmetic, so an edge of zero length never claims a point (0 / 0) and the point goes on to the vertex and edge tests
//    of the other two segments: a == b acts as the segment a c, and three equal vertices as the point a (region A: 0 <= 0).
//  * the interior's two ratios are clamped to the triangle (v in [0, 1], w in [0, 1 - v]); a NaN from 0 / 0 clamps to 0.  A face of
//    zero area with three distinct vertices has va = vb = vc = 0 and is claimed by the edge whose segment holds the point's projection
//    on the common line, or by a vertex: the nearest of its three segments.
// Every result is a point of the triangle spanned by the arguments: no rounding can make the distance smaller than the true one by
// more than the evaluation error of |ap - v e1 - w e2|^2.
#pragma once

template <class T> struct TriPoint {
    T b0, v, w;  // barycentrics of a, b, c: the closest point is a + v e1 + w e2
    T dist2;     // |p - closest|^2
};

template <class T> __device__ __forceinline__ T pt_fma(T a, T b, T c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float pt_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <class T> __device__ __forceinline__ T pt_dot(T ax, T ay, T az, T bx, T by, T bz) { return pt_fma(az, bz, pt_fma(ay, by, ax * bx)); }
template <class T> __device__ __forceinline__ T pt_clamp(T x, T lo, T hi) { return x > lo ? (x < hi ? x : hi) : lo; }  // NaN -> lo

// ap = p - a, e1 = b - a, e2 = c - a
template <class T>
__device__ __forceinline__ TriPoint<T> closest_on_triangle(T apx, T apy, T apz, T e1x, T e1y, T e1z, T e2x, T e2y, T e2z) {
#pragma clang fp contract(off)  // rounded as written, at either precision and in every kernel that includes this
    const T zero = T(0), one = T(1);
    const T bpx = apx - e1x, bpy = apy - e1y, bpz = apz - e1z;
    const T cpx = apx - e2x, cpy = apy - e2y, cpz = apz - e2z;
    const T d1 = pt_dot(e1x, e1y, e1z, apx, apy, apz), d2 = pt_dot(e2x, e2y, e2z, apx, apy, apz);
    const T d3 = pt_dot(e1x, e1y, e1z, bpx, bpy, bpz), d4 = pt_dot(e2x, e2y, e2z, bpx, bpy, bpz);
    const T d5 = pt_dot(e1x, e1y, e1z, cpx, cpy, cpz), d6 = pt_dot(e2x, e2y, e2z, cpx, cpy, cpz);
    const T vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const T ab_den = d1 - d3, ac_den = d2 - d6, bc_n = d4 - d3, bc_m = d5 - d6, bc_den = bc_n + bc_m;
    const bool in_a = (d1 <= zero) & (d2 <= zero);
    const bool in_b = (d3 >= zero) & (d4 <= d3);
    const bool in_ab = (vc <= zero) & (d1 >= zero) & (d3 <= zero) & (ab_den > zero);
    const bool in_c = (d6 >= zero) & (d5 <= d6);
    const bool in_ac = (vb <= zero) & (d2 >= zero) & (d6 <= zero) & (ac_den > zero);
    const bool in_bc = (va <= zero) & (bc_n >= zero) & (bc_m >= zero) & (bc_den > zero);
    // one reciprocal: the interior's, or that of the first edge region that holds
    const T den = in_ab ? ab_den : in_ac ? ac_den : in_bc ? bc_den : (va + vb) + vc;
    const T inv = one / den;
    T v = pt_clamp(vb * inv, zero, one), w;  // interior
    w = pt_clamp(vc * inv, zero, one - v);
    T b0 = (one - v) - w;
    if (in_bc) { w = pt_clamp(bc_n * inv, zero, one); v = one - w; b0 = zero; }
    if (in_ac) { w = pt_clamp(d2 * inv, zero, one); v = zero; b0 = one - w; }
    if (in_c) { v = zero; w = one; b0 = zero; }
    if (in_ab) { v = pt_clamp(d1 * inv, zero, one); w = zero; b0 = one - v; }
    if (in_b) { v = one; w = zero; b0 = zero; }
    if (in_a) { v = zero; w = zero; b0 = one; }
    const T rx = pt_fma(-w, e2x, pt_fma(-v, e1x, apx)), ry = pt_fma(-w, e2y, pt_fma(-v, e1y, apy)), rz = pt_fma(-w, e2z, pt_fma(-v, e1z, apz));
    TriPoint<T> r;
    r.b0 = b0; r.v = v; r.w = w;
    r.dist2 = pt_dot(rx, ry, rz, rx, ry, rz);
    return r;
}
