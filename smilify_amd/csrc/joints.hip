// Mesh-free joint kinematics for gfx950: the posed joints of SMAL.__call__ (reference smal_model/smal_torch.py:340-351) without a
// vertex, their backward, and the keypoint terms of a sequence fit fused onto both: the 3-D term (smil_kp3d_fit_eval) and the multi-view
// 2-D reprojection term with the 3-D one optionally beside it (smil_kp2d_fit_eval; specification: include/smilfit.h).
//
// A static-joint model's joints are the translation column of the kinematic chain.  A regressor model's joints are linear in the
// bone transforms: joints[j] = sum_k A_k m[j,k] over the (joint, bone) pairs of smilify_amd/joints.py, m = M0 + sum_b beta_b MB_b,
// J_rest = J0 + sum_b beta_b JB_b.  With A_k = [G_R | G_t - G_R J_k] a pair costs  G_R (m_xyz - J_k m_w) + G_t m_w.
//
// Decomposition: that of k_pose_fwd / k_chain_bwd (lbs.hip, "pose"): one wavefront per frame, lane = joint (NJ joints per lane for
// J > 64), everything a joint reads from memory waits in registers before the level loop, world transforms live in LDS while the
// chain is walked.  Arithmetic is float64 on float32 parameters; every output is rounded once.  The reverse walk GATHERS: a joint
// leaves what it owes its parent in its own LDS slot and the parent adds its children's slots in ascending order - no atomics.
// Blocks loop over frames (at most JT_MAX_BLOCKS blocks); the sums over frames of the shared tables' gradients (and of the fused
// term) are kept per wave in LDS in frame order, left as one row per block, and added in block order by the last block to finish.
#include <type_traits>

#include "chain.h"

#define JT_MAX_BLOCKS 1024
#define JT_MAX_FPB 4   // frames (waves) per block at the most

struct JArgs {
    SmilJointTables t;
    SmilJointsInputs in;
    int use_scale;
    float *joints, *new_J;  // forward outputs (joints: also the fused kernel's joints_out)
    const float *d_joints;
    float *d_beta, *d_theta, *d_trans, *d_logscale, *d_btrans;
    // fused 3-D keypoint term
    SmilFitConfig cfg;
    double w_k3d, sigma;
    int Jc;
    const int *canon;
    const float *target;
    const uint8_t *vis;
    const double *wj;
    float *objs;
    // fused multi-view 2-D keypoint term (K2D instantiations only; `target` / `vis` above are then the optional 3-D targets)
    double w_k2d, sigma_px;
    SmilCameras cam;
    int cam_wave;            // doubles of a wave's LDS that hold its frame's cameras; 0: one set per block, staged once, ...
    int cam_block;           // ... this many doubles behind the waves' LDS
    const float *target2d;   // (N,Nv,Jc,2) (y,x) px
    const uint8_t *vis2d;    // (N,Nv,Jc) or NULL
    const float *conf;       // (N,Nv,Jc) or NULL
    float *yx_out;           // (N,Nv,Jc,2) or NULL
    // sums over frames: columns of a block's row (-1: not kept), the rows and the counter of finished blocks
    int C, c_obj, c_obj2, c_beta, c_ls, c_bt;
    unsigned int *counter;
    double *part;
};

template <int NJ>
struct LaneState {
    int dep[NJ], par[NJ];
    double R[NJ][9], S[NJ][3], IS[NJ][3], T[NJ][3], TH[NJ][3];
};

// the moment of pair p for this frame's shape: m[0..2] = M0 + sum_b beta_b MB_b, m[3] = M0[3]
__device__ __forceinline__ void pair_moment(const JArgs &a, const float *__restrict__ beta, int p, double m[4]) {
    for (int c = 0; c < 4; ++c) m[c] = a.t.M0[4 * (size_t)p + c];
    const double *mb = a.t.MB + (size_t)p * a.t.nB * 3;
    for (int k = 0; k < a.in.nB_used; ++k) {
        const double bk = (double)beta[k];
        m[0] += bk * mb[3 * k]; m[1] += bk * mb[3 * k + 1]; m[2] += bk * mb[3 * k + 2];
    }
}

// Rest joints into sJ, the joints' local data into registers, then the level-synchronous walk: sG (J,12) world transforms.
// Called by every wave of the block (it synchronises the block); a wave without a frame (`live` false) only keeps step.
template <int NJ>
__device__ __forceinline__ void chain_forward(const JArgs &a, int b, bool live, int lane, const float *__restrict__ beta, double *sG,
                                              double *sJ, LaneState<NJ> &L) {
    const int J = a.t.J;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = lane + WAVE * q;
        if (live && j < J) {
            double x0 = a.t.J0[3 * j], x1 = a.t.J0[3 * j + 1], x2 = a.t.J0[3 * j + 2];
            for (int k = 0; k < a.in.nB_used; ++k) {
                const double bk = (double)beta[k];
                const double *jb = a.t.JB + ((size_t)k * J + j) * 3;
                x0 += bk * jb[0]; x1 += bk * jb[1]; x2 += bk * jb[2];
            }
            sJ[3 * j] = x0; sJ[3 * j + 1] = x1; sJ[3 * j + 2] = x2;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = lane + WAVE * q;
        L.dep[q] = -1; L.par[q] = 0;
        for (int k = 0; k < 3; ++k) { L.S[q][k] = 1.0; L.IS[q][k] = 1.0; L.T[q][k] = 0.0; L.TH[q][k] = 0.0; }
        for (int i = 0; i < 9; ++i) L.R[q][i] = 0.0;
        if (live && j < J) {
            L.dep[q] = a.t.depth[j];
            const float *th = a.in.theta + ((size_t)b * J + j) * 3;
            const float *mk = a.in.theta_mask ? a.in.theta_mask + 3 * j : nullptr;
            for (int k = 0; k < 3; ++k) L.TH[q][k] = mk ? (double)th[k] * (double)mk[k] : (double)th[k];
            rodrigues_fwd(L.TH[q], L.R[q]);
            const float *ls = a.use_scale ? a.in.logscale + (size_t)(a.in.logscale_shared ? 0 : b) * J * 3 : nullptr;
            if (ls)
                for (int k = 0; k < 3; ++k) L.S[q][k] = exp((double)ls[3 * j + k]);
            if (L.dep[q] > 0) {
                const int p = L.par[q] = a.t.parents[j];
                if (ls && !a.in.propagate_scaling)
                    for (int k = 0; k < 3; ++k) L.IS[q][k] = 1.0 / exp((double)ls[3 * p + k]);
                for (int k = 0; k < 3; ++k) L.T[q][k] = sJ[3 * j + k] - sJ[3 * p + k];
                if (a.in.btrans) {
                    const float *bt = a.in.btrans + ((size_t)(a.in.btrans_shared ? 0 : b) * J + j) * 3;
                    L.T[q][0] += (double)bt[0]; L.T[q][1] -= (double)bt[1]; L.T[q][2] += (double)bt[2];  // y flipped (batch_lbs.py:148)
                }
            }
        }
    }
    for (int d = 0; d <= a.t.max_depth; ++d) {
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
            if (L.dep[q] != d) continue;
            const int j = lane + WAVE * q;
            const double *R = L.R[q], *S = L.S[q], *isp = L.IS[q], *t = L.T[q];
            double G[12];
            if (d == 0) {
                chain_root(R, sJ + 3 * j, G);
            } else {
                double Lm[9];
                chain_local(isp, R, S, Lm);
                chain_compose(sG + 12 * L.par[q], Lm, t, G);
            }
            for (int i = 0; i < 12; ++i) sG[12 * j + i] = G[i];
        }
        __syncthreads();
    }
}

// factor of trans in joint j: 1 after the regression; before it the regressor's row sum, and nothing for a static-joint model
__device__ __forceinline__ double trans_factor(const JArgs &a, int j) {
    if (a.in.trans_after_joints) return 1.0;
    return a.t.static_joints ? 0.0 : a.t.rowsum[j];
}

// posed joint j of the frame whose chain lies in sG / sJ (without trans)
__device__ __forceinline__ void posed_joint(const JArgs &a, const float *__restrict__ beta, int j, const double *sG, const double *sJ,
                                            double out[3]) {
    if (a.t.static_joints) {
        out[0] = sG[12 * j + 3]; out[1] = sG[12 * j + 7]; out[2] = sG[12 * j + 11];
        return;
    }
    out[0] = out[1] = out[2] = 0.0;
    for (int p = a.t.pair_ptr[j]; p < a.t.pair_ptr[j + 1]; ++p) {
        const int k = a.t.pair_bone[p];
        double m[4];
        pair_moment(a, beta, p, m);
        const double *G = sG + 12 * k, *Jk = sJ + 3 * k;
        const double x0 = m[0] - Jk[0] * m[3], x1 = m[1] - Jk[1] * m[3], x2 = m[2] - Jk[2] * m[3];
        for (int r = 0; r < 3; ++r) out[r] += G[4 * r] * x0 + G[4 * r + 1] * x1 + G[4 * r + 2] * x2 + G[4 * r + 3] * m[3];
    }
}

template <int NJ>
__global__ void __launch_bounds__(64 * JT_MAX_FPB) k_joints_fwd(JArgs a) {
    extern __shared__ double smem64[];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fpb = blockDim.x >> 6;
    const int J = a.t.J, B = a.in.B;
    double *sG = smem64 + (size_t)wid * J * 15;  // (J,12) world transforms
    double *sJ = sG + J * 12;                     // (J,3) rest joints
    for (int b0 = blockIdx.x * fpb; b0 < B; b0 += gridDim.x * fpb) {
        const int b = b0 + wid;
        const bool live = b < B;
        const float *beta = a.in.beta + (size_t)(a.in.shared_beta || !live ? 0 : b) * a.in.nB_used;
        LaneState<NJ> L;
        chain_forward<NJ>(a, b, live, lane, beta, sG, sJ, L);
        double tr[3] = {0.0, 0.0, 0.0};
        if (live && a.in.trans)
            for (int k = 0; k < 3; ++k) tr[k] = (double)a.in.trans[3 * (size_t)b + k];
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
            const int j = lane + WAVE * q;
            if (!live || j >= J) continue;
            const size_t o = ((size_t)b * J + j) * 3;
            if (a.new_J) { a.new_J[o] = (float)sG[12 * j + 3]; a.new_J[o + 1] = (float)sG[12 * j + 7]; a.new_J[o + 2] = (float)sG[12 * j + 11]; }
            double x[3];
            posed_joint(a, beta, j, sG, sJ, x);
            const double f = trans_factor(a, j);
            for (int k = 0; k < 3; ++k) a.joints[o + k] = (float)(x[k] + f * tr[k]);
        }
        __syncthreads();  // (the next frame rewrites sG / sJ)
    }
}

// doubles of LDS a wave of the backward kernels needs: JT_BWD_ROW per joint (sG 12, sdG 12, 3 each of sJ sdJ sCt sCs sDJ), then its C sums
#define JT_BWD_ROW 39
__host__ __device__ static inline size_t bwd_wave_doubles(int J, int C) { return (size_t)J * JT_BWD_ROW + (size_t)C; }

// A camera staged for the 2-D term: sixteen doubles, float64 arithmetic on the float32 tables (camera.h: X_view = X R + T,
// k11 = 1 / tan(fov / 2), k00 = k11 / aspect, the principal point added after the division)
#define K2D_CAM 16
#define K2D_MAX_VIEWS 64
__device__ __forceinline__ void stage_camera64(double *row, const SmilCameras &c, int n) {
    const float *R = c.R + (size_t)(n % c.nR) * 9, *T = c.T + (size_t)(n % c.nT) * 3;
    for (int i = 0; i < 9; ++i) row[i] = (double)R[i];
    for (int i = 0; i < 3; ++i) row[9 + i] = (double)T[i];
    const double k11 = 1.0 / tan((double)c.fov[n % c.nFov] * 0.017453292519943295 / 2.0);
    row[12] = c.aspect ? k11 / (double)c.aspect[n % c.nAspect] : k11;
    row[13] = k11;
    row[14] = c.principal ? (double)c.principal[2 * (size_t)(n % c.nPrincipal)] : 0.0;
    row[15] = c.principal ? (double)c.principal[2 * (size_t)(n % c.nPrincipal) + 1] : 0.0;
}

// A squared residual s of weight w into `loss`; returns the weight of its gradient.  sigma > 0: soft L1,
// rho = 2 sigma^2 (u - 1) = 2 s / (u + 1), u = sqrt(1 + s / sigma^2), rho' = 1 / u; else the plain square.
__device__ __forceinline__ double robust_sq(double s, double w, double sigma, double &loss) {
    if (sigma > 0.0) {
        const double u = sqrt(1.0 + s / (sigma * sigma));
        loss += w * 2.0 * s / (u + 1.0);
        return w / u;
    }
    loss += w * s;
    return w;
}

// Backward of k_joints_fwd (FUSED false: d_joints from memory) and the fused keypoint evaluations (FUSED true: d_joints is the
// gradient of the term, formed here): the 3-D term alone (K2D false, smil_kp3d_fit_eval) or the multi-view 2-D term with the 3-D
// term optionally beside it (K2D true, smil_kp2d_fit_eval).  The forward is recomputed in LDS.  Everything the 2-D term adds
// stands under `if (K2D)`: the other instantiations hold the operations they held before it existed, in their order.
template <int NJ, bool FUSED, bool K2D = false>
__global__ void __launch_bounds__(64 * JT_MAX_FPB) k_joints_bwd(JArgs a) {
    static_assert(FUSED || !K2D, "the 2-D term is a fused term");
    extern __shared__ double smem64[];
    __shared__ unsigned int s_last;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fpb = blockDim.x >> 6;
    const int J = a.t.J, B = a.in.B, C = a.C;
    const size_t per_wave = bwd_wave_doubles(J, C) + (K2D ? (size_t)a.cam_wave : 0);
    double *sG = smem64 + (size_t)wid * per_wave;  // (J,12) world transforms
    double *sdG = sG + J * 12;                      // (J,12) their gradients; after a joint's turn: what it owes its parent
    double *sJ = sdG + J * 12;                      // (J,3) rest joints
    double *sdJ = sJ + J * 3;                       // (J,3) gradient on them
    double *sCt = sdJ + J * 3;                      // (J,3) dt of a joint: its parent's rest joint receives -dt
    double *sCs = sCt + J * 3;                      // (J,3) what a joint owes its parent's log scale
    double *sDJ = sCs + J * 3;                      // (J,3) upstream gradient on the posed joints
    double *acc = sDJ + J * 3;                      // (C) this wave's sums over its frames
    int *sChild = (int *)(smem64 + (size_t)fpb * per_wave);  // (J) the child lists, one copy per block
    for (int i = lane; i < C; i += WAVE) acc[i] = 0.0;
    for (int i = threadIdx.x; i < J - 1; i += blockDim.x) sChild[i] = a.t.child[i];
    // (K2D) the cameras of a frame, (views,16) float64: behind the wave's sums when they differ by frame, else behind the child lists
    double *sCam = K2D ? (a.cam_wave ? acc + C : smem64 + (size_t)fpb * per_wave + a.cam_block) : nullptr;
    if (K2D && !a.cam_wave)
        for (int v = threadIdx.x; v < a.cam.views; v += blockDim.x) stage_camera64(sCam + K2D_CAM * v, a.cam, v);
    __syncthreads();

    for (int b0 = blockIdx.x * fpb; b0 < B; b0 += gridDim.x * fpb) {
        const int b = b0 + wid;
        const bool live = b < B;
        const size_t fb = live ? b : 0;
        const float *beta = a.in.beta + (size_t)(a.in.shared_beta ? 0 : fb) * a.in.nB_used;
        LaneState<NJ> L;
        if (K2D && a.cam_wave && live && lane < a.cam.views)  // (visible after chain_forward's barriers)
            stage_camera64(sCam + K2D_CAM * lane, a.cam, (int)fb * a.cam.views + lane);
        chain_forward<NJ>(a, b, live, lane, beta, sG, sJ, L);

        // ---- upstream gradient on the posed joints ----
        bool dead = false;  // (wave-uniform) fused: nothing visible in this frame - every gradient is +0
        if (FUSED) {
            double loss = 0.0, nvis = 0.0;
            double loss2 = 0.0;  // (K2D) the 2-D term of this frame
            const double scale = live ? a.w_k3d / (3.0 * (double)a.Jc * (double)window_size_of(a.cfg, b)) : 0.0;
            constexpr int TERM_UNROLL = K2D ? 1 : NJ;  // (nothing below indexes the lane state: the 2-D term's longer body stays rolled, for the registers' sake)
#pragma unroll TERM_UNROLL
            for (int q = 0; q < NJ; ++q) {
                const int j = lane + WAVE * q;
                if (!live || j >= J) continue;
                double pos[3], dj[3] = {0.0, 0.0, 0.0};
                posed_joint(a, beta, j, sG, sJ, pos);
                if (a.in.trans)
                    for (int k = 0; k < 3; ++k) pos[k] += (double)a.in.trans[3 * fb + k];
                if (a.joints)
                    for (int k = 0; k < 3; ++k) a.joints[(fb * J + j) * 3 + k] = (float)pos[k];
                for (int c = 0; c < (K2D && !a.target ? 0 : a.Jc); ++c) {  // (every lane scans the list for its own joints: fixed order, duplicates allowed)
                    if ((a.canon ? a.canon[c] : c) != j) continue;
                    const float *tg = a.target + (fb * a.Jc + c) * 3;
                    const float t0 = tg[0], t1 = tg[1], t2 = tg[2];
                    const bool seen = (!a.vis || a.vis[fb * a.Jc + c] != 0) && isfinite(t0) && isfinite(t1) && isfinite(t2) &&
                                      !(t0 == 0.f && t1 == 0.f && t2 == 0.f);
                    if (!seen) continue;
                    const double w = (a.wj ? a.wj[c] : 1.0) * scale;
                    const double r0 = pos[0] - (double)t0, r1 = pos[1] - (double)t1, r2 = pos[2] - (double)t2;
                    const double s = r0 * r0 + r1 * r1 + r2 * r2;
                    const double g = robust_sq(s, w, a.sigma, loss);
                    dj[0] += 2.0 * g * r0; dj[1] += 2.0 * g * r1; dj[2] += 2.0 * g * r2;
                    nvis += 1.0;
                }
                if (K2D) {  // the 2-D term after the 3-D one: canon entries ascending, views ascending within each
                    const int Nv = a.cam.views;
                    const double hS = 0.5 * (double)a.cam.S;
                    const double scale2 = a.w_k2d / (2.0 * (double)a.Jc * (double)Nv * (double)window_size_of(a.cfg, b));
                    for (int c = 0; c < a.Jc; ++c) {
                        if ((a.canon ? a.canon[c] : c) != j) continue;
                        const double wc = (a.wj ? a.wj[c] : 1.0) * scale2;
                        for (int v = 0; v < Nv; ++v) {
                            const double *cm = sCam + K2D_CAM * v;
                            const size_t e = (fb * Nv + v) * a.Jc + c;
                            const double vx = pos[0] * cm[0] + pos[1] * cm[3] + pos[2] * cm[6] + cm[9];
                            const double vy = pos[0] * cm[1] + pos[1] * cm[4] + pos[2] * cm[7] + cm[10];
                            const double vz = pos[0] * cm[2] + pos[1] * cm[5] + pos[2] * cm[8] + cm[11];
                            const bool front = vz > (double)SMIL_ZNEAR;
                            const double iz = 1.0 / vz;
                            const double xn = vx * cm[12] * iz, yn = vy * cm[13] * iz;  // (unshifted)
                            const double ys = hS - hS * (yn + cm[15]), xs = hS - hS * (xn + cm[14]);
                            if (a.yx_out) {
                                a.yx_out[2 * e] = front ? (float)ys : __builtin_nanf("");
                                a.yx_out[2 * e + 1] = front ? (float)xs : __builtin_nanf("");
                            }
                            if (!a.target2d) continue;
                            const float ty = a.target2d[2 * e], tx = a.target2d[2 * e + 1];
                            const float cf = a.conf ? a.conf[e] : 1.f;
                            const bool seen = front && (!a.vis2d || a.vis2d[e] != 0) && isfinite(ty) && isfinite(tx) && isfinite(cf) && cf > 0.f;
                            if (!seen) continue;
                            const double w = wc * (double)cf;
                            const double ry = ys - (double)ty, rx = xs - (double)tx;
                            const double s = ry * ry + rx * rx;
                            const double g = robust_sq(s, w, a.sigma_px, loss2);
                            // d y_s = 2 g ry, d x_s = 2 g rx ; y_s = hS - hS y_ndc ; then camera_project_bwd's chain in float64
                            const double dyn = -hS * 2.0 * g * ry, dxn = -hS * 2.0 * g * rx;
                            const double dvx = dxn * cm[12] * iz, dvy = dyn * cm[13] * iz, dvz = -(xn * dxn + yn * dyn) * iz;
                            dj[0] += cm[0] * dvx + cm[1] * dvy + cm[2] * dvz;
                            dj[1] += cm[3] * dvx + cm[4] * dvy + cm[5] * dvz;
                            dj[2] += cm[6] * dvx + cm[7] * dvy + cm[8] * dvz;
                            nvis += 1.0;
                        }
                    }
                }
                for (int k = 0; k < 3; ++k) sDJ[3 * j + k] = dj[k];
            }
            loss = wave_sum(loss);
            nvis = wave_sum(nvis);
            dead = !(nvis > 0.0);
            if (K2D) {
                loss2 = wave_sum(loss2);
                if (lane == 0 && live && !dead) acc[a.c_obj2] += loss2;
            }
            if (lane == 0 && live && !dead) acc[a.c_obj] += loss;
        } else {
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                const int j = lane + WAVE * q;
                if (!live || j >= J) continue;
                for (int k = 0; k < 3; ++k) sDJ[3 * j + k] = (double)a.d_joints[(fb * J + j) * 3 + k];
            }
        }
        __syncthreads();

        // ---- gradient on the world transforms, gathered by bone ----
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
            const int j = lane + WAVE * q;
            if (!live || j >= J) continue;
            double dA[12];
            for (int i = 0; i < 12; ++i) dA[i] = 0.0;
            if (!a.t.static_joints) {
                for (int e = a.t.bpair_ptr[j]; e < a.t.bpair_ptr[j + 1]; ++e) {
                    const int jj = a.t.bpair_joint[e];
                    double m[4];
                    pair_moment(a, beta, a.t.bpair_index[e], m);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 4; ++c) dA[4 * r + c] += sDJ[3 * jj + r] * m[c];
                }
            }
            const double *G = sG + 12 * j, *Jj = sJ + 3 * j;
            for (int r = 0; r < 3; ++r) {  // A_R = G_R ; A_t = G_t - G_R J
                const double dt = dA[4 * r + 3];
                for (int c = 0; c < 3; ++c) sdG[12 * j + 4 * r + c] = dA[4 * r + c] - dt * Jj[c];
                sdG[12 * j + 4 * r + 3] = dt + (a.t.static_joints ? sDJ[3 * j + r] : 0.0);
            }
            for (int n = 0; n < 3; ++n) sdJ[3 * j + n] = -(G[n] * dA[3] + G[4 + n] * dA[7] + G[8 + n] * dA[11]);
        }
        __syncthreads();

        // ---- reverse walk ----
        for (int d = a.t.max_depth; d >= 0; --d) {
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                if (L.dep[q] != d) continue;
                const int j = lane + WAVE * q;
                const size_t o = fb * J + j;
                double dG[12], dJ[3], dSp[3] = {0.0, 0.0, 0.0};
                for (int i = 0; i < 12; ++i) dG[i] = sdG[12 * j + i];
                for (int k = 0; k < 3; ++k) dJ[k] = sdJ[3 * j + k];
                for (int e = a.t.child_ptr[j]; e < a.t.child_ptr[j + 1]; ++e) {  // children, ascending: what each owes this joint
                    const int c = sChild[e];
                    for (int i = 0; i < 12; ++i) dG[i] += sdG[12 * c + i];
                    for (int k = 0; k < 3; ++k) { dJ[k] -= sCt[3 * c + k]; dSp[k] += sCs[3 * c + k]; }
                }
                double dR[9], dS[3] = {0.0, 0.0, 0.0}, dbt[3] = {0.0, 0.0, 0.0};
                if (d == 0) {
                    for (int m = 0; m < 3; ++m) {
                        dR[3 * m] = dG[4 * m]; dR[3 * m + 1] = dG[4 * m + 1]; dR[3 * m + 2] = dG[4 * m + 2];
                        dJ[m] += dG[4 * m + 3];
                    }
                } else {
                    const double *R = L.R[q], *S = L.S[q], *isp = L.IS[q], *t = L.T[q];
                    double Lm[9];
                    for (int m = 0; m < 3; ++m)
                        for (int n = 0; n < 3; ++n) Lm[3 * m + n] = (isp[m] * R[3 * m + n]) * S[n];
                    const double *P = sG + 12 * L.par[q];
                    // owed to the parent: dGp_R += dG_R L^T + dG_t (x) t ; dGp_t += dG_t
                    for (int m = 0; m < 3; ++m) {
                        for (int k = 0; k < 3; ++k)
                            sdG[12 * j + 4 * m + k] = dG[4 * m] * Lm[3 * k] + dG[4 * m + 1] * Lm[3 * k + 1] + dG[4 * m + 2] * Lm[3 * k + 2] +
                                                      dG[4 * m + 3] * t[k];
                        sdG[12 * j + 4 * m + 3] = dG[4 * m + 3];
                    }
                    // local: dL = Gp_R^T dG_R ; dt = Gp_R^T dG_t
                    double dL[9], dt[3];
                    for (int k = 0; k < 3; ++k) {
                        for (int n = 0; n < 3; ++n) dL[3 * k + n] = P[k] * dG[n] + P[4 + k] * dG[4 + n] + P[8 + k] * dG[8 + n];
                        dt[k] = P[k] * dG[3] + P[4 + k] * dG[7] + P[8 + k] * dG[11];
                    }
                    for (int k = 0; k < 3; ++k) { dJ[k] += dt[k]; sCt[3 * j + k] = dt[k]; }
                    dbt[0] = dt[0]; dbt[1] = -dt[1]; dbt[2] = dt[2];
                    for (int m = 0; m < 3; ++m) {
                        double dis = 0.0;  // sum_n L[m][n] dL[m][n]: minus the parent's log-scale gradient, row m
                        for (int n = 0; n < 3; ++n) {
                            dR[3 * m + n] = isp[m] * dL[3 * m + n] * S[n];
                            dis += Lm[3 * m + n] * dL[3 * m + n];
                        }
                        sCs[3 * j + m] = (a.use_scale && !a.in.propagate_scaling) ? -dis : 0.0;
                    }
                    if (a.use_scale)
                        for (int n = 0; n < 3; ++n) dS[n] = Lm[n] * dL[n] + Lm[3 + n] * dL[3 + n] + Lm[6 + n] * dL[6 + n];
                }
                for (int k = 0; k < 3; ++k) sdJ[3 * j + k] = dJ[k];
                if (a.d_theta) {
                    double dth[3];
                    rodrigues_bwd(L.TH[q], dR, dth);
                    for (int k = 0; k < 3; ++k) a.d_theta[o * 3 + k] = dead ? 0.f : (float)dth[k];
                }
                if (a.d_logscale) {
                    for (int k = 0; k < 3; ++k) {
                        const double v = a.use_scale ? dS[k] + dSp[k] : 0.0;
                        if (a.c_ls >= 0) { if (!dead) acc[a.c_ls + 3 * j + k] += v; }
                        else a.d_logscale[o * 3 + k] = dead ? 0.f : (float)v;
                    }
                }
                if (a.d_btrans) {
                    for (int k = 0; k < 3; ++k) {
                        const double v = a.in.btrans ? dbt[k] : 0.0;
                        if (a.c_bt >= 0) { if (!dead) acc[a.c_bt + 3 * j + k] += v; }
                        else a.d_btrans[o * 3 + k] = dead ? 0.f : (float)v;
                    }
                }
            }
            __syncthreads();
        }

        // ---- translation and shape ----
        if (a.d_trans) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                const int j = lane + WAVE * q;
                if (!live || j >= J) continue;
                const double f = a.in.trans ? trans_factor(a, j) : 0.0;
                s0 += f * sDJ[3 * j]; s1 += f * sDJ[3 * j + 1]; s2 += f * sDJ[3 * j + 2];
            }
            s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
            if (lane == 0 && live) {
                a.d_trans[3 * fb] = dead ? 0.f : (float)s0; a.d_trans[3 * fb + 1] = dead ? 0.f : (float)s1;
                a.d_trans[3 * fb + 2] = dead ? 0.f : (float)s2;
            }
        }
        if (a.d_beta) {
            for (int k = 0; k < a.in.nB_used; ++k) {
                double r = 0.0;
#pragma unroll
                for (int q = 0; q < NJ; ++q) {
                    const int j = lane + WAVE * q;
                    if (!live || j >= J) continue;
                    const double *jb = a.t.JB + ((size_t)k * J + j) * 3;  // through the rest joints ...
                    r += sdJ[3 * j] * jb[0] + sdJ[3 * j + 1] * jb[1] + sdJ[3 * j + 2] * jb[2];
                    if (a.t.static_joints) continue;
                    const double *G = sG + 12 * j;                         // ... and through the moments of this bone's pairs
                    for (int e = a.t.bpair_ptr[j]; e < a.t.bpair_ptr[j + 1]; ++e) {
                        const double *dj = sDJ + 3 * a.t.bpair_joint[e];
                        const double *mb = a.t.MB + ((size_t)a.t.bpair_index[e] * a.t.nB + k) * 3;
                        for (int c = 0; c < 3; ++c) r += (G[c] * dj[0] + G[4 + c] * dj[1] + G[8 + c] * dj[2]) * mb[c];
                    }
                }
                r = wave_sum(r);
                if (lane == 0 && live) {
                    if (a.c_beta >= 0) { if (!dead) acc[a.c_beta + k] += r; }
                    else a.d_beta[fb * a.in.nB_used + k] = dead ? 0.f : (float)r;
                }
            }
        }
        __syncthreads();  // (the next frame rewrites the tables)
    }

    // ---- sums over frames: the block's row, then - in the last block to finish - the rows in block order ----
    if (C == 0) return;  // (uniform)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0;
        for (int w = 0; w < fpb; ++w) s += smem64[(size_t)w * per_wave + (size_t)J * JT_BWD_ROW + c];
        __hip_atomic_store(&a.part[(size_t)blockIdx.x * C + c], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();  // this block's row is visible device-wide before it counts as done
        s_last = atomicAdd(a.counter, 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;  // (uniform)
    __threadfence();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0;
        for (unsigned int blk = 0; blk < gridDim.x; ++blk)
            s += __hip_atomic_load(&a.part[(size_t)blk * C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (K2D && c == a.c_obj2) { if (a.target2d) a.objs[0] += (float)s; }
        else if (K2D && c == a.c_obj) { if (a.target) a.objs[9] += (float)s; }
        else if (c == a.c_obj) a.objs[9] += (float)s;
        else if (a.c_beta >= 0 && c >= a.c_beta && c < a.c_beta + a.in.nB_used) a.d_beta[c - a.c_beta] = (float)s;
        else if (a.c_ls >= 0 && c >= a.c_ls && c < a.c_ls + 3 * J) a.d_logscale[c - a.c_ls] = (float)s;
        else if (a.c_bt >= 0 && c >= a.c_bt && c < a.c_bt + 3 * J) a.d_btrans[c - a.c_bt] = (float)s;
    }
    if (threadIdx.x == 0) *a.counter = 0u;  // (the next call on this workspace starts from zero)
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static int check_joint_args(const char *who, const SmilJointTables *t, const SmilJointsInputs *in) {
    SMIL_REQUIRE(t && in, "%s: null argument", who);
    SMIL_REQUIRE(t->J >= 1 && t->J <= SMIL_MAX_JOINTS, "%s: J=%d outside 1..%d", who, t->J, SMIL_MAX_JOINTS);
    SMIL_REQUIRE(t->nB >= 0 && t->nB <= SMIL_MAX_BETAS && t->P >= 0 && t->max_depth >= 0 && t->max_depth < t->J, "%s: bad table sizes", who);
    SMIL_REQUIRE(t->parents && t->depth && t->child_ptr && (t->child || t->J == 1) && t->J0 && (t->JB || t->nB == 0),
                 "%s: a chain table is missing", who);
    SMIL_REQUIRE(t->static_joints ? t->P == 0 : (t->pair_ptr && t->bpair_ptr && t->rowsum && (t->P == 0 || (t->pair_bone && t->M0 &&
                 t->bpair_joint && t->bpair_index && (t->MB || t->nB == 0)))), "%s: a pair table is missing (P=%d)", who, t->P);
    SMIL_REQUIRE(in->B >= 1, "%s: B=%d", who, in->B);
    SMIL_REQUIRE(in->nB_used >= 0 && in->nB_used <= t->nB, "%s: nB_used=%d but the model has %d shape directions", who, in->nB_used, t->nB);
    SMIL_REQUIRE(in->beta || in->nB_used == 0, "%s: beta is missing", who);
    SMIL_REQUIRE(in->theta, "%s: theta is missing", who);
    return SMIL_OK;
}

static int frames_per_block(size_t wave_bytes, size_t block_bytes) {
    const size_t budget = 64 * 1024;
    if (wave_bytes + block_bytes >= budget) return 1;
    return (int)std::min<size_t>(JT_MAX_FPB, (budget - block_bytes) / wave_bytes);
}

template <class K>
static int launch_joints(K kern, const JArgs &a, size_t wave_bytes, size_t block_bytes, hipStream_t stream) {
    const int fpb = frames_per_block(wave_bytes, block_bytes);
    const size_t lds = fpb * wave_bytes + block_bytes;
    SMIL_REQUIRE(lds <= smil_device_limits().lds_block, "joints: %zu bytes of LDS per workgroup exceed the device's %zu", lds,
                 smil_device_limits().lds_block);
    if (lds > 64 * 1024) SMIL_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = std::min(ceil_div(a.in.B, fpb), JT_MAX_BLOCKS);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * fpb), lds, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// f(std::integral_constant<int, NJ>) for the joints per lane that J asks for
template <class F>
static int dispatch_nj(int J, F f) {
    if (J <= WAVE) return f(std::integral_constant<int, 1>());
    if (J <= 2 * WAVE) return f(std::integral_constant<int, 2>());
    if (J <= 3 * WAVE) return f(std::integral_constant<int, 3>());
    return f(std::integral_constant<int, 4>());
}

// bytes of LDS: the 2-D term's cameras (per wave when a table has a row per image, else once per block), and a backward kernel's in all
struct CamLds { size_t wave = 0, block = 0; };
struct BwdLdsBytes { size_t wave, block, child; };
static BwdLdsBytes bwd_lds_bytes(int J, int C, const CamLds &cl) {
    const size_t child = align256((size_t)J * sizeof(int));
    return {bwd_wave_doubles(J, C) * sizeof(double) + cl.wave, child + cl.block, child};
}
static int joints_grid(const SmilJointTables *t, const SmilJointsInputs *in, int C, const CamLds &cl = CamLds()) {
    const BwdLdsBytes lb = bwd_lds_bytes(t->J, C, cl);
    return std::min(ceil_div(in->B, frames_per_block(lb.wave, lb.block)), JT_MAX_BLOCKS);
}

// columns of the rows that hold the sums over frames
struct SumColumns { int C = 0, c_obj = -1, c_obj2 = -1, c_beta = -1, c_ls = -1, c_bt = -1; };
static SumColumns sum_columns(const SmilJointTables *t, const SmilJointsInputs *in, bool obj, bool beta, bool ls, bool bt, bool obj2 = false) {
    SumColumns s;
    if (obj) { s.c_obj = s.C; s.C += 1; }
    if (obj2) { s.c_obj2 = s.C; s.C += 1; }
    if (beta && in->shared_beta && in->nB_used > 0) { s.c_beta = s.C; s.C += in->nB_used; }
    if (ls && in->logscale_shared) { s.c_ls = s.C; s.C += 3 * t->J; }
    if (bt && in->btrans_shared) { s.c_bt = s.C; s.C += 3 * t->J; }
    return s;
}
static size_t sums_workspace(const SmilJointTables *t, const SmilJointsInputs *in, const SumColumns &s, const CamLds &cl = CamLds()) {
    if (s.C == 0) return 0;
    return 256 + align256((size_t)joints_grid(t, in, s.C, cl) * s.C * sizeof(double));  // [counter | rows]
}

// what every entry point sets of the kernels' arguments
static void joint_args(const SmilJointTables *t, const SmilJointsInputs *in, JArgs &a) {
    a = {};
    a.t = *t; a.in = *in;
    a.use_scale = in->logscale && in->allow_limb_scaling;
}

extern "C" int smil_joints_forward(const SmilJointTables *t, const SmilJointsInputs *in, float *joints, float *new_J, void *stream_) {
    if (int rc = check_joint_args("smil_joints_forward", t, in)) return rc;
    SMIL_REQUIRE(joints, "smil_joints_forward: joints is missing");
    JArgs a;
    joint_args(t, in, a);
    a.joints = joints; a.new_J = new_J;
    const size_t wave = (size_t)t->J * 15 * sizeof(double);
    return dispatch_nj(t->J, [&](auto nj) { return launch_joints(k_joints_fwd<decltype(nj)::value>, a, wave, 0, (hipStream_t)stream_); });
}

template <bool FUSED, bool K2D = false>
static int launch_bwd(JArgs &a, const SumColumns &sc, void *workspace, hipStream_t s, const CamLds &cl = CamLds()) {
    a.C = sc.C; a.c_obj = sc.c_obj; a.c_obj2 = sc.c_obj2; a.c_beta = sc.c_beta; a.c_ls = sc.c_ls; a.c_bt = sc.c_bt;
    if (sc.C) {
        a.counter = (unsigned int *)workspace;
        a.part = (double *)((char *)workspace + 256);
    }
    const BwdLdsBytes lb = bwd_lds_bytes(a.t.J, sc.C, cl);
    a.cam_wave = (int)(cl.wave / sizeof(double)); a.cam_block = (int)(lb.child / sizeof(double));
    return dispatch_nj(a.t.J, [&](auto nj) {
        return launch_joints(k_joints_bwd<decltype(nj)::value, FUSED, K2D>, a, lb.wave, lb.block, s);
    });
}

extern "C" size_t smil_joints_backward_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, const SmilJointsGrads *g) {
    if (!t || !in || !g || t->J < 1 || in->B < 1) return 0;
    return sums_workspace(t, in, sum_columns(t, in, false, g->d_beta != nullptr, g->d_logscale != nullptr, g->d_btrans != nullptr));
}

extern "C" int smil_joints_backward(const SmilJointTables *t, const SmilJointsInputs *in, const SmilJointsGrads *g, void *stream_) {
    if (int rc = check_joint_args("smil_joints_backward", t, in)) return rc;
    SMIL_REQUIRE(g && g->d_joints, "smil_joints_backward: d_joints is missing");
    const SumColumns sc = sum_columns(t, in, false, g->d_beta != nullptr, g->d_logscale != nullptr, g->d_btrans != nullptr);
    SMIL_REQUIRE(sc.C == 0 || g->workspace, "smil_joints_backward: the gradient of a shared table needs the workspace");
    JArgs a;
    joint_args(t, in, a);
    a.d_joints = g->d_joints;
    a.d_beta = in->nB_used > 0 ? g->d_beta : nullptr;
    a.d_theta = g->d_theta; a.d_trans = g->d_trans; a.d_logscale = g->d_logscale; a.d_btrans = g->d_btrans;
    return launch_bwd<false>(a, sc, g->workspace, (hipStream_t)stream_);
}

// the checks, in their order (`present`: the caller's own pointers that must not be null), and the arguments the fused entry points share
struct FitEvalOut { float *objs, *d_pose, *d_trans, *d_betas, *d_logscale, *d_btrans, *joints_out; void *workspace; };
static int fit_eval_args(const char *who, const SmilFitConfig *cfg, const SmilJointTables *t, const SmilJointsInputs *in, int32_t Jc,
                         const int32_t *canon, const double *joint_weights, double w_k3d, double robust_scale, bool present,
                         const FitEvalOut &o, JArgs &a) {
    if (int rc = check_joint_args(who, t, in)) return rc;
    SMIL_REQUIRE(cfg && present && o.objs && o.workspace, "%s: null argument", who);
    SMIL_REQUIRE(cfg->N == in->B && cfg->J == t->J, "%s: cfg holds N=%d J=%d, the inputs B=%d J=%d", who, cfg->N, cfg->J, in->B, t->J);
    SMIL_REQUIRE(cfg->frame0 >= 0 && cfg->N_total >= cfg->frame0 + cfg->N, "%s: bad frame range", who);
    SMIL_REQUIRE(Jc >= 1, "%s: Jc=%d", who, Jc);
    SMIL_REQUIRE(canon || Jc <= t->J, "%s: Jc=%d above J=%d without a canon list", who, Jc, t->J);
    joint_args(t, in, a);
    a.joints = o.joints_out;
    a.d_beta = in->nB_used > 0 ? o.d_betas : nullptr;
    a.d_theta = o.d_pose; a.d_trans = o.d_trans; a.d_logscale = o.d_logscale; a.d_btrans = o.d_btrans;
    a.cfg = *cfg; a.w_k3d = w_k3d; a.sigma = robust_scale;
    a.Jc = Jc; a.canon = canon; a.wj = joint_weights; a.objs = o.objs;
    return SMIL_OK;
}

extern "C" size_t smil_kp3d_fit_eval_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, int32_t want_betas,
                                                     int32_t want_logscale, int32_t want_btrans) {
    if (!t || !in || t->J < 1 || in->B < 1) return 0;
    return sums_workspace(t, in, sum_columns(t, in, true, want_betas != 0, want_logscale != 0, want_btrans != 0));
}

extern "C" int smil_kp3d_fit_eval(const SmilFitConfig *cfg, double w_k3d, double robust_scale, const SmilJointTables *t,
                                  const SmilJointsInputs *in, int32_t Jc, const int32_t *canon, const float *target,
                                  const uint8_t *visibility, const double *joint_weights, float *objs, float *d_pose, float *d_trans,
                                  float *d_betas, float *d_logscale, float *d_btrans, float *joints_out, void *workspace, void *stream_) {
    JArgs a;
    if (int rc = fit_eval_args("smil_kp3d_fit_eval", cfg, t, in, Jc, canon, joint_weights, w_k3d, robust_scale, target != nullptr,
                               {objs, d_pose, d_trans, d_betas, d_logscale, d_btrans, joints_out, workspace}, a)) return rc;
    SMIL_REQUIRE(in->trans_after_joints, "smil_kp3d_fit_eval: the term is defined on the fitter convention (trans_after_joints = 1)");
    SMIL_REQUIRE(std::isfinite(w_k3d) && std::isfinite(robust_scale) && robust_scale >= 0.0,
                 "smil_kp3d_fit_eval: w_k3d=%g robust_scale=%g", w_k3d, robust_scale);
    const SumColumns sc = sum_columns(t, in, true, d_betas != nullptr, d_logscale != nullptr, d_btrans != nullptr);
    a.target = target; a.vis = visibility;
    return launch_bwd<true>(a, sc, workspace, (hipStream_t)stream_);
}

// ---- the multi-view 2-D keypoint term (with the 3-D term optionally beside it) ----
static int check_kp2d_cameras(const SmilCameras *cam, int N, CamLds *cl) {
    SMIL_REQUIRE(cam && cam->R && cam->T && cam->fov, "smil_kp2d_fit_eval: a camera table is missing");
    SMIL_REQUIRE(cam->views >= 1 && cam->views <= K2D_MAX_VIEWS, "smil_kp2d_fit_eval: views=%d outside 1..%d", cam->views, K2D_MAX_VIEWS);
    SMIL_REQUIRE((long long)cam->N == (long long)N * cam->views, "smil_kp2d_fit_eval: cameras hold N=%d images, expected %d frames x %d views",
                 cam->N, N, cam->views);
    SMIL_REQUIRE(cam->S >= 1, "smil_kp2d_fit_eval: S=%d", cam->S);
    const int rows[5] = {cam->nR, cam->nT, cam->nFov, cam->aspect ? cam->nAspect : 1, cam->principal ? cam->nPrincipal : 1};
    const char *names[5] = {"R", "T", "fov", "aspect", "principal"};
    bool per_frame = false;
    for (int k = 0; k < 5; ++k) {
        SMIL_REQUIRE(rows[k] == 1 || rows[k] == cam->views || rows[k] == cam->N,
                     "smil_kp2d_fit_eval: camera table %s has %d rows; expected 1, views=%d or N*views=%d", names[k], rows[k], cam->views, cam->N);
        per_frame = per_frame || rows[k] > cam->views;
    }
    const size_t bytes = (size_t)cam->views * K2D_CAM * sizeof(double);
    *cl = CamLds();
    if (per_frame) cl->wave = bytes; else cl->block = bytes;
    return SMIL_OK;
}

extern "C" size_t smil_kp2d_fit_eval_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, const SmilCameras *cam,
                                                     int32_t want_betas, int32_t want_logscale, int32_t want_btrans) {
    if (!t || !in || !cam || t->J < 1 || in->B < 1) return 0;
    CamLds cl;
    if (check_kp2d_cameras(cam, in->B, &cl)) return 0;
    return sums_workspace(t, in, sum_columns(t, in, true, want_betas != 0, want_logscale != 0, want_btrans != 0, true), cl);
}

extern "C" int smil_kp2d_fit_eval(const SmilFitConfig *cfg, double w_k2d, double robust_scale_px, const SmilJointTables *t,
                                  const SmilJointsInputs *in, const SmilCameras *cam, int32_t Jc, const int32_t *canon,
                                  const float *target2d, const uint8_t *visibility2d, const float *confidence, const double *joint_weights,
                                  double w_k3d, double robust_scale, const float *target3d, const uint8_t *visibility3d, float *objs,
                                  float *d_pose, float *d_trans, float *d_betas, float *d_logscale, float *d_btrans, float *joints_out,
                                  float *yx_out, void *workspace, void *stream_) {
    JArgs a;
    if (int rc = fit_eval_args("smil_kp2d_fit_eval", cfg, t, in, Jc, canon, joint_weights, w_k3d, robust_scale, true,
                               {objs, d_pose, d_trans, d_betas, d_logscale, d_btrans, joints_out, workspace}, a)) return rc;
    SMIL_REQUIRE(in->trans_after_joints == 1, "smil_kp2d_fit_eval: the term is defined on the fitter convention (trans_after_joints = 1)");
    SMIL_REQUIRE(std::isfinite(w_k2d) && w_k2d >= 0.0 && std::isfinite(robust_scale_px) && robust_scale_px >= 0.0 && std::isfinite(w_k3d) &&
                 w_k3d >= 0.0 && std::isfinite(robust_scale) && robust_scale >= 0.0,
                 "smil_kp2d_fit_eval: w_k2d=%g robust_scale_px=%g w_k3d=%g robust_scale=%g must be finite and not negative", w_k2d,
                 robust_scale_px, w_k3d, robust_scale);
    CamLds cl;
    if (int rc = check_kp2d_cameras(cam, cfg->N, &cl)) return rc;
    const bool has2d = target2d && w_k2d > 0.0, has3d = target3d && w_k3d > 0.0;
    SMIL_REQUIRE(has2d || has3d, "smil_kp2d_fit_eval: neither term is asked for (w_k2d=%g with%s 2-D targets, w_k3d=%g with%s 3-D targets)",
                 w_k2d, target2d ? "" : "out", w_k3d, target3d ? "" : "out");
    const SumColumns sc = sum_columns(t, in, true, d_betas != nullptr, d_logscale != nullptr, d_btrans != nullptr, true);
    a.target = has3d ? target3d : nullptr; a.vis = visibility3d;
    a.w_k2d = w_k2d; a.sigma_px = robust_scale_px; a.cam = *cam;
    a.target2d = has2d ? target2d : nullptr; a.vis2d = visibility2d; a.conf = confidence; a.yx_out = yx_out;
    return launch_bwd<true, true>(a, sc, workspace, (hipStream_t)stream_, cl);
}
