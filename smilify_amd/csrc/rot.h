// Rotation conversions (rotations.hip): the arithmetic of the 6-D representation, axis-angle and rotation matrices, stated ONCE.
// Every map is a forward function that fills a small struct of what it computed on the way and a backward function that reads the
// same struct, so the forward, backward and fused kernels evaluate the same expressions.  All of it is float64 whatever the storage
// type.  The maps are those of pytorch3d.transforms (rotation_6d_to_matrix, axis_angle_to_matrix, matrix_to_axis_angle) as
// include/smilfit.h states them; they are NOT chain.h's Rodrigues, which carries the reference model's +1e-8 on the angle.
//
// Derivative conventions (torch autograd's, which the backward functions reproduce): the norm of a zero vector has derivative 0,
// max(x, eps) passes the gradient where x >= eps, and the square root of a non-positive number is 0 with derivative 0.
//
// Contraction is off from here on: with IEEE +, -, *, /, sqrt evaluated in the order written, the results are the reference
// evaluation's up to the last bits of sin, cos and atan2 and the order of three-term sums - a fused multiply-add would change which
// bits cancel in the difference of two nearly equal matrices (the distance of close rotations).  The kernels are memory- and
// launch-bound; the instructions this costs are not on their critical path.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)
#define ROT_FN __host__ __device__ __forceinline__  // (host too: the arithmetic can be exercised without a device)

#define ROT_NORM_EPS 1e-12     // the clamp under a normalisation (torch.nn.functional.normalize's eps)
#define ROT_QUAT_FLOOR 0.1     // the floor under the quaternion candidate's divisor
#define ROT_SERIES_BELOW 0.05  // |h| below which sin(h) / (2 h) and its derivative are Taylor series

ROT_FN double rot_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ROT_FN void rot_cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// g(h) = sin(h) / (2 h), continued to 1/2 at h = 0, and g'(h), from h, sin(h) and cos(h).  Below ROT_SERIES_BELOW both are series
// whose first neglected terms are h^10 / 79833600 and h^9 / 6652800: the quotient form of g' cancels to -h^3 / 3 there.
ROT_FN void rot_half_sinc(double h, double sin_h, double cos_h, double &g, double &dg) {
    if (fabs(h) < ROT_SERIES_BELOW) {
        const double h2 = h * h;
        g = 0.5 - h2 * (1.0 / 12.0 - h2 * (1.0 / 240.0 - h2 * (1.0 / 10080.0 - h2 * (1.0 / 725760.0))));
        dg = -h * (1.0 / 6.0 - h2 * (1.0 / 60.0 - h2 * (1.0 / 1680.0 - h2 * (1.0 / 90720.0))));
    } else {
        g = sin_h / (2.0 * h);
        dg = (h * cos_h - sin_h) / (2.0 * h * h);
    }
}

// ---- b = a / max(|a|, eps) ----
struct RotUnit {
    double b[3];
    double n, c;  // |a| and the divisor max(|a|, eps)
};
ROT_FN void rot_unit_fwd(const double *a, RotUnit &s) {
    s.n = sqrt(rot_dot3(a, a));
    s.c = fmax(s.n, ROT_NORM_EPS);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.b[k] = a[k] / s.c;
}
ROT_FN void rot_unit_bwd(const double *a, const RotUnit &s, const double *gb, double *ga) {
    const double gc = -rot_dot3(gb, s.b) / s.c;
    const double gn_over_n = (s.n >= ROT_NORM_EPS && s.n > 0.0) ? gc / s.n : 0.0;  // through the clamp and the norm
#pragma unroll
    for (int k = 0; k < 3; ++k) ga[k] = gb[k] / s.c + gn_over_n * a[k];
}

// ---- 6-D -> matrix: Gram-Schmidt of a1 = d[0:3], a2 = d[3:6]; the rows of R are b1, b2, b1 x b2 ----
struct Rot6d {
    RotUnit u1, u2;  // b1 of a1, b2 of u
    double d, u[3];  // d = b1 . a2, u = a2 - d b1
    double R[9];
};
ROT_FN void rot6d_fwd(const double *a, Rot6d &s) {
    const double *a2 = a + 3;
    rot_unit_fwd(a, s.u1);
    s.d = rot_dot3(s.u1.b, a2);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.u[k] = a2[k] - s.d * s.u1.b[k];
    rot_unit_fwd(s.u, s.u2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.R[k] = s.u1.b[k];
        s.R[3 + k] = s.u2.b[k];
    }
    rot_cross3(s.u1.b, s.u2.b, s.R + 6);
}
ROT_FN void rot6d_bwd(const double *a, const Rot6d &s, const double *gR, double *ga) {
    const double *a2 = a + 3, *b1 = s.u1.b, *b2 = s.u2.b, *g3 = gR + 6;
    double gb1[3], gb2[3], t[3], gu[3];
    rot_cross3(b2, g3, t);  // b3 = b1 x b2
#pragma unroll
    for (int k = 0; k < 3; ++k) gb1[k] = gR[k] + t[k];
    rot_cross3(g3, b1, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) gb2[k] = gR[3 + k] + t[k];
    rot_unit_bwd(s.u, s.u2, gb2, gu);
    const double gd = -rot_dot3(gu, b1);  // u = a2 - d b1, d = b1 . a2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gb1[k] += gd * a2[k] - s.d * gu[k];
        ga[3 + k] = gu[k] + gd * b1[k];
    }
    rot_unit_bwd(a, s.u1, gb1, ga);
}

// ---- the matrix of a quaternion q = (r, i, j, k) of any length, t = 2 / (q . q) ----
ROT_FN void rot_quat_matrix(const double *q, double t, double *R) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    R[0] = 1.0 - t * (j * j + k * k); R[1] = t * (i * j - k * r);       R[2] = t * (i * k + j * r);
    R[3] = t * (i * j + k * r);       R[4] = 1.0 - t * (i * i + k * k); R[5] = t * (j * k - i * r);
    R[6] = t * (i * k - j * r);       R[7] = t * (j * k + i * r);       R[8] = 1.0 - t * (i * i + j * j);
}
// gq = the gradient on q through the entries AND through t
ROT_FN void rot_quat_matrix_bwd(const double *q, double t, const double *g, double *gq) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    const double gt = -(g[0] * (j * j + k * k) + g[4] * (i * i + k * k) + g[8] * (i * i + j * j)) + g[1] * (i * j - k * r) +
                      g[2] * (i * k + j * r) + g[3] * (i * j + k * r) + g[5] * (j * k - i * r) + g[6] * (i * k - j * r) + g[7] * (j * k + i * r);
    const double w = -gt * t * t;  // d t / d q = -t^2 q
    gq[0] = t * (k * (g[3] - g[1]) + j * (g[2] - g[6]) + i * (g[7] - g[5])) + w * r;
    gq[1] = t * (-2.0 * i * (g[4] + g[8]) + j * (g[1] + g[3]) + k * (g[2] + g[6]) + r * (g[7] - g[5])) + w * i;
    gq[2] = t * (-2.0 * j * (g[0] + g[8]) + i * (g[1] + g[3]) + k * (g[5] + g[7]) + r * (g[2] - g[6])) + w * j;
    gq[3] = t * (-2.0 * k * (g[0] + g[4]) + i * (g[2] + g[6]) + j * (g[5] + g[7]) + r * (g[3] - g[1])) + w * k;
}

// ---- axis-angle -> matrix: q = (cos(theta / 2), a g(theta / 2)), theta = |a| ----
struct RotAa {
    double theta, sin_h, g, dg;  // of h = theta / 2
    double q[4], t;
};
ROT_FN void rot_aa_fwd(const double *a, RotAa &s, double *R) {
    s.theta = sqrt(rot_dot3(a, a));
    const double h = 0.5 * s.theta;
    double cos_h;
    sincos(h, &s.sin_h, &cos_h);
    rot_half_sinc(h, s.sin_h, cos_h, s.g, s.dg);
    s.q[0] = cos_h;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.q[1 + k] = a[k] * s.g;
    s.t = 2.0 / (s.q[0] * s.q[0] + s.q[1] * s.q[1] + s.q[2] * s.q[2] + s.q[3] * s.q[3]);
    rot_quat_matrix(s.q, s.t, R);
}
ROT_FN void rot_aa_bwd(const double *a, const RotAa &s, const double *gR, double *ga) {
    double gq[4];
    rot_quat_matrix_bwd(s.q, s.t, gR, gq);
    const double gh = -s.sin_h * gq[0] + s.dg * rot_dot3(a, gq + 1);
    const double gtheta_over_theta = s.theta > 0.0 ? 0.5 * gh / s.theta : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ga[k] = s.g * gq[1 + k] + gtheta_over_theta * a[k];
}

// ---- matrix -> axis-angle through the quaternion candidate of the largest qa (any 3 x 3 input) ----
// The four candidates are the rows of the symmetric matrix K with the diagonal x_i = qa_i^2 and, above it,
//   K01 = m21 - m12, K02 = m02 - m20, K03 = m10 - m01, K12 = m10 + m01, K13 = m02 + m20, K23 = m12 + m21.
// The x_i add up to 4, so the largest qa is >= 1 for every finite input: the floor never binds on the chosen row.
struct RotMat {
    int c;                     // the chosen candidate
    double qa, den, sign;      // its qa, the divisor 2 max(qa, floor), -1 where the quaternion was negated
    double q[4];               // the standardised quaternion
    double n, g, dg;           // |q[1:]|, g and g' at h = atan2(n, q0)
};
ROT_FN void rot_mat_fwd(const double *m, RotMat &s, double *aa) {
    const double x[4] = {1.0 + m[0] + m[4] + m[8], 1.0 + m[0] - m[4] - m[8], 1.0 - m[0] + m[4] - m[8], 1.0 - m[0] - m[4] + m[8]};
    s.c = 0;
    s.qa = x[0] > 0.0 ? sqrt(x[0]) : 0.0;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double qi = x[i] > 0.0 ? sqrt(x[i]) : 0.0;
        if (qi > s.qa) {  // (a tie keeps the lowest index)
            s.qa = qi;
            s.c = i;
        }
    }
    const double k01 = m[7] - m[5], k02 = m[2] - m[6], k03 = m[3] - m[1], k12 = m[3] + m[1], k13 = m[2] + m[6], k23 = m[5] + m[7];
    const double kcc = s.qa * s.qa;
    const int c = s.c;
    const double num[4] = {c == 0 ? kcc : c == 1 ? k01 : c == 2 ? k02 : k03, c == 0 ? k01 : c == 1 ? kcc : c == 2 ? k12 : k13,
                           c == 0 ? k02 : c == 1 ? k12 : c == 2 ? kcc : k23, c == 0 ? k03 : c == 1 ? k13 : c == 2 ? k23 : kcc};
    s.den = 2.0 * fmax(s.qa, ROT_QUAT_FLOOR);
    s.sign = num[0] / s.den < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s.q[i] = s.sign * (num[i] / s.den);
    s.n = sqrt(rot_dot3(s.q + 1, s.q + 1));
    const double h = atan2(s.n, s.q[0]);
    double sin_h, cos_h;
    sincos(h, &sin_h, &cos_h);
    rot_half_sinc(h, sin_h, cos_h, s.g, s.dg);
#pragma unroll
    for (int k = 0; k < 3; ++k) aa[k] = s.q[1 + k] / s.g;
}
ROT_FN void rot_mat_bwd(const RotMat &s, const double *gaa, double *gm) {
    // aa = v / g(h), h = atan2(n, q0), n = |v|
    const double *v = s.q + 1;
    const double gh = -rot_dot3(gaa, v) / (s.g * s.g) * s.dg;
    const double rr = s.n * s.n + s.q[0] * s.q[0];
    const double gn_over_n = s.n > 0.0 ? gh * s.q[0] / rr / s.n : 0.0;
    double gq[4];
    gq[0] = -gh * s.n / rr;
#pragma unroll
    for (int k = 0; k < 3; ++k) gq[1 + k] = gaa[k] / s.g + gn_over_n * v[k];
    // q = sign num / den
    double gnum[4], gden = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        gnum[i] = s.sign * gq[i] / s.den;
        gden -= gq[i] * s.q[i] / s.den;
    }
    // den = 2 max(qa, floor), K_cc = qa^2, qa = sqrt(x_c)
    const int c = s.c;
    const double gkcc = c == 0 ? gnum[0] : c == 1 ? gnum[1] : c == 2 ? gnum[2] : gnum[3];
    const double gqa = (s.qa >= ROT_QUAT_FLOOR ? 2.0 * gden : 0.0) + 2.0 * s.qa * gkcc;
    const double gx = s.qa > 0.0 ? gqa / (2.0 * s.qa) : 0.0;
    gm[0] = (c <= 1 ? gx : -gx);
    gm[4] = (c == 0 || c == 2 ? gx : -gx);
    gm[8] = (c == 0 || c == 3 ? gx : -gx);
    // row c of K: entry K_ab (a < b) is num[b] where c == a and num[a] where c == b
    const double g01 = c == 0 ? gnum[1] : c == 1 ? gnum[0] : 0.0, g02 = c == 0 ? gnum[2] : c == 2 ? gnum[0] : 0.0;
    const double g03 = c == 0 ? gnum[3] : c == 3 ? gnum[0] : 0.0, g12 = c == 1 ? gnum[2] : c == 2 ? gnum[1] : 0.0;
    const double g13 = c == 1 ? gnum[3] : c == 3 ? gnum[1] : 0.0, g23 = c == 2 ? gnum[3] : c == 3 ? gnum[2] : 0.0;
    gm[7] = g01 + g23; gm[5] = g23 - g01;
    gm[2] = g02 + g13; gm[6] = g13 - g02;
    gm[3] = g03 + g12; gm[1] = g12 - g03;
}

// ---- the Frobenius distance of two matrices; gD = d dist / d (Rp - Rt), 0 where dist == 0 (torch's convention for the norm) ----
ROT_FN double rot_frobenius(const double *Rp, const double *Rt, double *D) {
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        D[k] = Rp[k] - Rt[k];
        ss += D[k] * D[k];
    }
    return sqrt(ss);
}
