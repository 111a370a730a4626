// Where a face can leave a record: the rounded blur box (included by raster_common.h; tests/test_raster_rounded_boxes_cpu.py compiles
// it into a stand-alone host program, so nothing here is a HIP type and the function qualifier is a macro).
//
// A (face, pixel) pair becomes a record iff the pixel centre is inside the face or eval_pair2's squared distance to the face is below
// `blur`.  Let [fx0, fx1] x [fy0, fy1] be the face's unblurred bounding box.  A centre inside the face is inside that box; a centre
// outside the face is at least as far from the face as from the box.  So for a run of pixel columns [i_lo, i_hi] and rows
// [j_lo, j_hi], with dx = max(0, fx0 - c(i_hi), c(i_lo) - fx1) the gap between the box and the nearest centre of the run (dy
// likewise), no pixel of the run holds a record unless dx^2 + dy^2 < blur: the region that can hold one is the bounding box with
// ROUNDED corners, not the square the pixel boxes of k_raster_setup and stage_faces cover.
//
// Units and slack.  Everything here is in pixels on the flipped axis, where pixel index i has its centre at coordinate i and the NDC
// coordinate c sits at v(c) = ((c + 1) S - 1) / 2 (the same map the pixel boxes use).  The reach is sqrt(blur) S / 2 pixels and the
// test is dx^2 + dy^2 < (reach + REACH_SLACK_PX)^2: the 0.01 px that the pixel boxes add on either side, added to the radius.
// What the slack has to cover, for S <= 2048 (TILE * 256) and coordinates of the order of the image:
//  * v(c) rounds three times (c + 1, x S, - 1) at magnitudes up to S: <= 3 ulp(2048) / 2 = 3.7e-4 px;
//  * eval_pair2 works relative to the tile centre in NDC, vertices and pixel centres rounded at magnitude <= 2 (ulp 2.4e-7, x S / 2 =
//    2.4e-4 px), and its projections, squares and sum add a few ulp of a distance that is itself below the reach: together well under
//    1e-3 px of distance;
//  * reach^2 against `blur` itself (the kernels are handed sqrtf(blur)), the squares and the sum here, the square root of the trim
//    (1 ulp): relative 1e-6 of at most 16 px.
// Less than 2e-3 px in all, against 1e-2.  A face far outside the image (the front part of a cut face) has huge coordinates and
// huge rounding errors in proportion - and gaps that are larger still: v(c) is monotone, so a gap only vanishes where the exact one
// does.  Infinite coordinates give infinite gaps (never a NaN: the face's finiteness is checked before).
#pragma once
#include <math.h>

#ifndef REACH_FN
#define REACH_FN static inline
#endif
#define REACH_SLACK_PX 0.01f
#ifdef __HIP_DEVICE_COMPILE__
#define REACH_SQRT(x) __builtin_amdgcn_sqrtf(x)  // v_sqrt_f32, 1 ulp (sqrtf is a dozen instructions and a branch for its last bit)
#else
#define REACH_SQRT(x) sqrtf(x)
#endif

// pixel coordinate (flipped axis) of the NDC coordinate c
REACH_FN float reach_px_of(float c, float fS) { return ((c + 1.0f) * fS - 1.0f) * 0.5f; }
// (reach + slack)^2 in pixels^2
REACH_FN float reach_limit2(float sqrt_blur, float fS) {
    const float r = sqrt_blur * fS * 0.5f + REACH_SLACK_PX;
    return r * r;
}
// gap between the extent [vlo, vhi] and the nearest centre of the pixels i_lo .. i_hi
REACH_FN float reach_gap(float vlo, float vhi, int i_lo, int i_hi) { return fmaxf(fmaxf(vlo - (float)i_hi, (float)i_lo - vhi), 0.0f); }
// can a run of pixels with these gaps hold a record?
REACH_FN bool reach_holds(float dx, float dy, float lim2) { return dx * dx + dy * dy < lim2; }

// Cuts the pixels i_lo .. i_hi of one axis to those that can hold a record when the other axis is at least `d_other` away: the gap
// on this axis must stay below sqrt(lim2 - d_other^2).  An empty result is i_hi < i_lo.  (Clamped in float before the conversion:
// the extent of a cut face's front part can lie far outside the int range.)
REACH_FN void reach_trim(float vlo, float vhi, float d_other, float lim2, int &i_lo, int &i_hi) {
    const float rr = lim2 - d_other * d_other;
    if (!(rr > 0.0f)) { i_hi = i_lo - 1; return; }
    const float w = REACH_SQRT(rr);
    const float lo = fminf(fmaxf(ceilf(vlo - w), (float)i_lo), (float)i_hi + 1.0f);
    const float hi = fmaxf(fminf(floorf(vhi + w), (float)i_hi), (float)i_lo - 1.0f);
    i_lo = (int)lo;
    i_hi = (int)hi;
}

// The four corner tiles of a face's tile box (tx0 .. tx1) x (ty0 .. ty1), tiles of `tile` pixels in OUTPUT order (output column xo
// holds pixel index S - 1 - xo).  (xo0 .. xo1) x (yo0 .. yo1) is the face's pixel box in output order, [vx0, vx1] x [vy0, vy1] its
// unblurred extent in pixel coordinates.  Bit (2 cy + cx) of the result is set when the tile (cx ? tx1 : tx0, cy ? ty1 : ty0)
// cannot hold a record of the face: the part of the pixel box inside it fails reach_holds.  Every flag is worked out for its own
// tile and used for that tile alone (reach_corner_culled), so a flag is right whatever the reach; that ONLY corners can fail - an
// edge tile has dx or dy = 0 - holds while the reach is at most one tile, and the callers cull nothing beyond that.
REACH_FN unsigned reach_corner_flags(float vx0, float vx1, float vy0, float vy1, int xo0, int xo1, int yo0, int yo1,
                                     int tx0, int tx1, int ty0, int ty1, int S, int tile, float lim2) {
    float dx[2], dy[2];
    for (int c = 0; c < 2; ++c) {
        const int tx = c ? tx1 : tx0, ty = c ? ty1 : ty0;
        const int xa = xo0 > tx * tile ? xo0 : tx * tile, xb = xo1 < tx * tile + tile - 1 ? xo1 : tx * tile + tile - 1;
        const int ya = yo0 > ty * tile ? yo0 : ty * tile, yb = yo1 < ty * tile + tile - 1 ? yo1 : ty * tile + tile - 1;
        dx[c] = reach_gap(vx0, vx1, S - 1 - xb, S - 1 - xa);
        dy[c] = reach_gap(vy0, vy1, S - 1 - yb, S - 1 - ya);
    }
    return (reach_holds(dx[0], dy[0], lim2) ? 0u : 1u) | (reach_holds(dx[1], dy[0], lim2) ? 0u : 2u) |
           (reach_holds(dx[0], dy[1], lim2) ? 0u : 4u) | (reach_holds(dx[1], dy[1], lim2) ? 0u : 8u);
}
REACH_FN bool reach_corner_culled(unsigned flags, int tx, int ty, int tx0, int tx1, int ty0, int ty1) {
    const bool ex = tx == tx0 || tx == tx1, ey = ty == ty0 || ty == ty1;
    return ex && ey && ((flags >> ((ty == ty1 ? 2 : 0) + (tx == tx1 ? 1 : 0))) & 1u) != 0u;
}
