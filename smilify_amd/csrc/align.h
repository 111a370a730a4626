// The per-problem arithmetic of the 3-D alignment kernels (align.hip), float64, on values that are already in registers: Horn's
// 4 x 4 matrix, its eigen-decomposition by cyclic Jacobi, the transform of the top eigenvector and the closed-form gradient.  The
// formulas are stated at include/smilfit.h.  Every loop has constant bounds and is unrolled: the arrays stay in registers.
// The functions are __host__ __device__ so that a host program can run the same expressions.
#pragma once
#include <cmath>

#define ALIGN_HD __host__ __device__ __forceinline__

// weighted moments of one problem: W = sum w, the weighted means, and on the centred points M[3 a + b] = sum w x_a y_b,
// vx = sum w |x|^2
struct AlignMoments {
    double W, mx[3], my[3], M[9], vx;
};
// eigenvalues lam[0] >= ... >= lam[3] of N and their eigenvectors, v[4 k + i] component i of eigenvector k
struct AlignEig {
    double lam[4], v[16];
};
// the transform y = s R x + t of one problem (R row-major), its eigenvalue gap and status
struct AlignTransform {
    double R[9], t[3], s, gap;
    int status;
};

// N (4 x 4, row-major, both triangles) of S (3 x 3, row-major); linear in S
ALIGN_HD void align_horn(const double *S, double *N) {
    const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
    N[0] = xx + yy + zz;
    N[5] = xx - yy - zz;
    N[10] = -xx + yy - zz;
    N[15] = -xx - yy + zz;
    N[1] = N[4] = yz - zy;
    N[2] = N[8] = zx - xz;
    N[3] = N[12] = xy - yx;
    N[6] = N[9] = xy + yx;
    N[7] = N[13] = zx + xz;
    N[11] = N[14] = yz + zy;
}

// the adjoint of align_horn: gS[3 a + b] = sum_ij G[4 i + j] dN[i][j] / dS[a][b] for any 4 x 4 G
ALIGN_HD void align_horn_adjoint(const double *G, double *gS) {
    const double d0 = G[0], d1 = G[5], d2 = G[10], d3 = G[15];
    const double h01 = G[1] + G[4], h02 = G[2] + G[8], h03 = G[3] + G[12], h12 = G[6] + G[9], h13 = G[7] + G[13], h23 = G[11] + G[14];
    gS[0] = d0 + d1 - d2 - d3;
    gS[4] = d0 - d1 + d2 - d3;
    gS[8] = d0 - d1 - d2 + d3;
    gS[1] = h03 + h12;
    gS[3] = -h03 + h12;
    gS[5] = h01 + h23;
    gS[7] = -h01 + h23;
    gS[6] = h02 + h13;
    gS[2] = -h02 + h13;
}

ALIGN_HD void align_swap_pair(AlignEig &e, int i, int j) {  // (i, j constants at every call)
    if (e.lam[i] < e.lam[j]) {
        double x = e.lam[i];
        e.lam[i] = e.lam[j];
        e.lam[j] = x;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            x = e.v[4 * i + r];
            e.v[4 * i + r] = e.v[4 * j + r];
            e.v[4 * j + r] = x;
        }
    }
}

// Cyclic Jacobi on the symmetric a (4 x 4, row-major, both triangles; destroyed): at most 12 sweeps, ended when the off-diagonal sum
// of squares is at most (2^-52 Frobenius norm)^2.  A pivot that is zero, or that does not change either of its diagonal entries when
// a hundred times itself is added, is set to zero and skipped.
ALIGN_HD void align_jacobi4(double *a, AlignEig &e) {
    double v[16];  // v[4 r + k]: component r of column k
    double frob = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        v[i] = (i % 5 == 0) ? 1.0 : 0.0;
        frob += a[i] * a[i];
    }
    const double tol = 4.930380657631324e-32 * frob;  // (2^-52)^2 |a|_F^2
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += 2.0 * a[4 * p + q] * a[4 * p + q];
        if (off <= tol) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[4 * p + q], app = a[4 * p + p], aqq = a[4 * q + q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    a[4 * p + q] = a[4 * q + p] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[4 * p + p] = app - t * apq;
                a[4 * q + q] = aqq + t * apq;
                a[4 * p + q] = a[4 * q + p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r != p && r != q) {
                        const double arp = a[4 * r + p], arq = a[4 * r + q];
                        a[4 * r + p] = a[4 * p + r] = c * arp - s * arq;
                        a[4 * r + q] = a[4 * q + r] = s * arp + c * arq;
                    }
                    const double vrp = v[4 * r + p], vrq = v[4 * r + q];
                    v[4 * r + p] = c * vrp - s * vrq;
                    v[4 * r + q] = s * vrp + c * vrq;
                }
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e.lam[k] = a[5 * k];
#pragma unroll
        for (int r = 0; r < 4; ++r) e.v[4 * k + r] = v[4 * r + k];
    }
    align_swap_pair(e, 0, 1);  // a sorting network on four, descending
    align_swap_pair(e, 2, 3);
    align_swap_pair(e, 0, 2);
    align_swap_pair(e, 1, 3);
    align_swap_pair(e, 1, 2);
}

// the rotation of the quaternion q = (a, b, c, d), |q| = 1; even in q
ALIGN_HD void align_quat_matrix(const double *q, double *R) {
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    R[0] = a * a + b * b - c * c - d * d;
    R[1] = 2.0 * (b * c - a * d);
    R[2] = 2.0 * (b * d + a * c);
    R[3] = 2.0 * (b * c + a * d);
    R[4] = a * a - b * b + c * c - d * d;
    R[5] = 2.0 * (c * d - a * b);
    R[6] = 2.0 * (b * d - a * c);
    R[7] = 2.0 * (c * d + a * b);
    R[8] = a * a - b * b - c * c + d * d;
}

// sum_ab R[a][b] M[b][a]: the weighted sum of y . R x over the centred points
ALIGN_HD double align_trace_RM(const double *R, const double *M) {
    double c = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) c += R[3 * a + b] * M[3 * b + a];
    return c;
}

// The solve of one problem from its moments: the eigen-decomposition in `e`, the transform and the status in `x`.
ALIGN_HD void align_solve(const AlignMoments &m, int with_scale, double min_gap, AlignEig &e, AlignTransform &x) {
#pragma unroll
    for (int k = 0; k < 9; ++k) x.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    x.s = 1.0;
    x.gap = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) e.lam[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) e.v[k] = 0.0;
    if (!(m.W > 0.0)) {
        x.status = SMIL_ALIGN_EMPTY;
        x.t[0] = x.t[1] = x.t[2] = 0.0;
        return;
    }
    double N[16];
    align_horn(m.M, N);
    align_jacobi4(N, e);
    const double big = fmax(e.lam[0], -e.lam[3]);
    if (big > 0.0) x.gap = (e.lam[0] - e.lam[1]) / big;
    // (written so that a NaN gap, from moments that overflowed, is degenerate too)
    if (m.vx == 0.0 || !(big > 0.0) || !(x.gap > min_gap)) {
        x.status = SMIL_ALIGN_DEGENERATE;
#pragma unroll
        for (int k = 0; k < 3; ++k) x.t[k] = m.my[k] - m.mx[k];
        return;
    }
    x.status = SMIL_ALIGN_OK;
    align_quat_matrix(e.v, x.R);
    if (with_scale) x.s = align_trace_RM(x.R, m.M) / m.vx;
#pragma unroll
    for (int a = 0; a < 3; ++a) x.t[a] = m.my[a] - x.s * (x.R[3 * a] * m.mx[0] + x.R[3 * a + 1] * m.mx[1] + x.R[3 * a + 2] * m.mx[2]);
}

// The gradient of one SMIL_ALIGN_OK problem on its moments from the upstream gR (9), gt (3), gs: gM (9), g_vx, g_mx (3), g_my (3).
// gR is the caller's copy and is changed.
ALIGN_HD void align_solve_backward(const AlignEig &e, const double *mx, const double *M, double vx, double s, int with_scale, double *gR,
                                   const double *gt, double gs, double *gM, double &g_vx, double *g_mx, double *g_my) {
    double R[9];
    align_quat_matrix(e.v, R);
    // t = my - s R mx
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g_my[a] = gt[a];
        gs -= gt[a] * (R[3 * a] * mx[0] + R[3 * a + 1] * mx[1] + R[3 * a + 2] * mx[2]);
        g_mx[a] = -s * (R[a] * gt[0] + R[3 + a] * gt[1] + R[6 + a] * gt[2]);
#pragma unroll
        for (int b = 0; b < 3; ++b) gR[3 * a + b] -= s * gt[a] * mx[b];
    }
    // s = sum_ab R[a][b] M[b][a] / vx
    g_vx = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) gM[k] = 0.0;
    if (with_scale) {
        const double f = gs / vx;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                gR[3 * a + b] += f * M[3 * b + a];
                gM[3 * b + a] = f * R[3 * a + b];
            }
        g_vx = -f * s;
    }
    // sum gR R(q) = q^T N(gR^T) q, so gq = 2 N(gR^T) q
    double gRt[9], Ng[16], gq[4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) gRt[3 * a + b] = gR[3 * b + a];
    align_horn(gRt, Ng);
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = 2.0 * (Ng[4 * i] * e.v[0] + Ng[4 * i + 1] * e.v[1] + Ng[4 * i + 2] * e.v[2] + Ng[4 * i + 3] * e.v[3]);
    // dq = sum_k v_k (v_k . dN q) / (lam_1 - lam_k): the gradient on N is G = u q^T
    double u[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const double *vk = e.v + 4 * k;
        const double f = (vk[0] * gq[0] + vk[1] * gq[1] + vk[2] * gq[2] + vk[3] * gq[3]) / (e.lam[0] - e.lam[k]);
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] += f * vk[i];
    }
    double G[16], gS[9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) G[4 * i + j] = u[i] * e.v[j];
    align_horn_adjoint(G, gS);
#pragma unroll
    for (int k = 0; k < 9; ++k) gM[k] += gS[k];
}
