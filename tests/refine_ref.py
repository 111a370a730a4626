"""float64 numpy restatement of the camera refinement (csrc/refine.hip; reference smal_fitter/sleap_data/refine_camera_params.py
:143-226) for the CPU and GPU tests: the Rodrigues rotation and its derivative, one accumulation (cost, g, H of scipy's soft_l1 on
every scalar residual, analytic Jacobian), the kernel's exact Levenberg-Marquardt rules, and a 40-digit mpmath evaluation of the same
accumulation."""
import os

import numpy as np

import lm_ref
from lm_ref import rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_POINTS = 20
CONVERGED, STEP_LIMIT, SKIPPED, NONFINITE = 0, 1, 2, 3
GEN = np.zeros((3, 3, 3))  # GEN[k] = [e_k]x
for _k, (_i, _j) in enumerate(((2, 1), (0, 2), (1, 0))):
    GEN[_k, _i, _j], GEN[_k, _j, _i] = 1.0, -1.0


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "refine_cameras_ref.npz")))


def correspondences(fx):
    """[(pts_3d, pts_2d)] per camera of the fixture."""
    o = fx["offsets"]
    return [(fx["pts_3d"][o[c]:o[c + 1]], fx["pts_2d"][o[c]:o[c + 1]]) for c in range(len(o) - 1)]


def names(fx):
    return [f"cam{c:02d}" for c in range(len(fx["counts"]))]


def camera_of(params10):
    from smilify_amd import refine_cameras as rc

    p = np.asarray(params10, np.float64)
    K = np.array([[p[6], 0.0, p[8]], [0.0, p[7], p[9]], [0.0, 0.0, 1.0]])
    return dict(K=K, dist=np.zeros(5), R=rc.rodrigues(p[:3]), t=p[3:6].reshape(3, 1).copy(), rvec=p[:3].copy())


def coefficients(t2):
    """a = sin(th)/th, b = (1 - cos(th))/th^2, a1 = (cos(th) - a)/th^2, b1 = (a - 2 b)/th^2; series below th^2 = 1e-3."""
    if t2 < 1e-3:
        return (1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 - t2 / 5040.0)), 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 - t2 / 40320.0)),
                -1.0 / 3.0 + t2 * (1.0 / 30.0 + t2 * (-1.0 / 840.0 + t2 / 45360.0)),
                -1.0 / 12.0 + t2 * (1.0 / 180.0 + t2 * (-1.0 / 6720.0 + t2 / 453600.0)))
    th = np.sqrt(t2)
    a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t2
    return a, b, (np.cos(th) - a) / t2, (a - 2.0 * b) / t2


def rodrigues(r):
    """R (3, 3) and dR (3, 3, 3), dR[k] = dR / dr_k."""
    r = np.asarray(r, np.float64)
    a, b, a1, b1 = coefficients(float(r @ r))
    K = np.einsum("k,kij->ij", r, GEN)
    K2 = K @ K
    dR = np.stack([r[k] * (a1 * K + b1 * K2) + a * GEN[k] + b * (GEN[k] @ K + K @ GEN[k]) for k in range(3)])
    return np.eye(3) + a * K + b * K2, dR


def jacobian(params10, p3):
    """The projections (M, 2) and the Jacobian rows Ju, Jv (M, 10) of u = fx x / z + cx, v = fy y / z + cy."""
    p = np.asarray(params10, np.float64)
    R, dR = rodrigues(p[:3])
    with np.errstate(all="ignore"):
        Xc = p3 @ R.T + p[3:6]
        iz = 1.0 / Xc[:, 2]
        xn, yn = Xc[:, 0] * iz, Xc[:, 1] * iz
        M = len(p3)
        du = np.stack([p[6] * iz, np.zeros(M), -p[6] * xn * iz], axis=1)  # d u / d Xc
        dv = np.stack([np.zeros(M), p[7] * iz, -p[7] * yn * iz], axis=1)
        D = np.einsum("kij,mj->mki", dR, p3)  # d Xc / d r_k
        Ju, Jv = np.zeros((M, 10)), np.zeros((M, 10))
        Ju[:, :3], Jv[:, :3] = np.einsum("mi,mki->mk", du, D), np.einsum("mi,mki->mk", dv, D)
        Ju[:, 3:6], Jv[:, 3:6] = du, dv
        Ju[:, 6], Ju[:, 8], Jv[:, 7], Jv[:, 9] = xn, 1.0, yn, 1.0
        proj = np.stack([p[6] * xn + p[8], p[7] * yn + p[9]], axis=1)
    return proj, Ju, Jv


def evaluate(params10, p3, p2, n_params=10, f_scale=5.0):
    """cost, g (10), H (10, 10) in float64; entries outside the n_params block are zero."""
    proj, Ju, Jv = jacobian(params10, p3)
    Ju[:, n_params:], Jv[:, n_params:] = 0.0, 0.0
    with np.errstate(all="ignore"):
        f = proj - p2
        z = (f / f_scale) ** 2
        cost = 0.5 * f_scale ** 2 * float(np.sum(2.0 * (np.sqrt(1.0 + z) - 1.0)))  # as scipy writes it
        w = 1.0 / np.sqrt(1.0 + z)
        g = Ju.T @ (w[:, 0] * f[:, 0]) + Jv.T @ (w[:, 1] * f[:, 1])
        H = Ju.T @ (w[:, 0:1] * Ju) + Jv.T @ (w[:, 1:2] * Jv)
    return cost, g, H


def evaluate_mp(params10, p3, p2, f_scale=5.0, digits=40, rounded=True):
    """The same accumulation (10 parameters) in `digits`-digit arithmetic, with the closed-form Rodrigues coefficients (their limits
    at th = 0), rounded to float64.  The 6-parameter values are its leading blocks.  rounded=False: the unrounded mpf values, cost, g as
    a list and the symmetric H as a list of rows (for lm_ref.lm_exact)."""
    import mpmath as mp

    with mp.workprec(int(digits * 3.33) + 8):
        p = [mp.mpf(float(v)) for v in params10]
        r = p[:3]
        t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
        if t2 == 0:
            a, b, a1, b1 = mp.mpf(1), mp.mpf(1) / 2, -mp.mpf(1) / 3, -mp.mpf(1) / 12
        else:
            th = mp.sqrt(t2)
            a, b = mp.sin(th) / th, (1 - mp.cos(th)) / t2
            a1, b1 = (mp.cos(th) - a) / t2, (a - 2 * b) / t2
        gen = [mp.matrix(GEN[k].tolist()) for k in range(3)]
        K = r[0] * gen[0] + r[1] * gen[1] + r[2] * gen[2]
        K2 = K * K
        R = mp.eye(3) + a * K + b * K2
        dR = [r[k] * (a1 * K + b1 * K2) + a * gen[k] + b * (gen[k] * K + K * gen[k]) for k in range(3)]
        fs = mp.mpf(float(f_scale))
        cost, g, H = mp.mpf(0), [mp.mpf(0)] * 10, [[mp.mpf(0)] * 10 for _ in range(10)]
        zero, one = mp.mpf(0), mp.mpf(1)
        for X, o in zip(np.asarray(p3, np.float64).tolist(), np.asarray(p2, np.float64).tolist()):
            X = [mp.mpf(v) for v in X]
            Xc = [R[i, 0] * X[0] + R[i, 1] * X[1] + R[i, 2] * X[2] + p[3 + i] for i in range(3)]
            iz = one / Xc[2]
            xn, yn = Xc[0] * iz, Xc[1] * iz
            du, dv = [p[6] * iz, zero, -p[6] * xn * iz], [zero, p[7] * iz, -p[7] * yn * iz]
            D = [[dR[k][i, 0] * X[0] + dR[k][i, 1] * X[1] + dR[k][i, 2] * X[2] for i in range(3)] for k in range(3)]
            Ju = [du[0] * D[k][0] + du[2] * D[k][2] for k in range(3)] + du + [xn, zero, one, zero]
            Jv = [dv[1] * D[k][1] + dv[2] * D[k][2] for k in range(3)] + dv + [zero, yn, zero, one]
            for f, J in ((p[6] * xn + p[8] - mp.mpf(o[0]), Ju), (p[7] * yn + p[9] - mp.mpf(o[1]), Jv)):
                h = mp.sqrt(1 + (f / fs) ** 2)
                cost += 2 * (h - 1)
                w = one / h
                nz = [i for i in range(10) if J[i] != 0]
                for i in nz:
                    g[i] += J[i] * w * f
                    wi = w * J[i]
                    for j in nz:
                        if j >= i:
                            H[i][j] += wi * J[j]
        cost = fs * fs * cost / 2
        if not rounded:
            return cost, g, [[H[min(i, j)][max(i, j)] for j in range(10)] for i in range(10)]
        Hf = np.array([[float(H[min(i, j)][max(i, j)]) for j in range(10)] for i in range(10)])
        return float(cost), np.array([float(v) for v in g]), Hf


def block(g, H, n_params):
    """g and H with everything outside the n_params block zeroed."""
    g, H = g.copy(), H.copy()
    g[n_params:], H[n_params:], H[:, n_params:] = 0.0, 0.0, 0.0
    return g, H


def lm(params10, p3, p2, n_params=10, f_scale=5.0, max_steps=100):
    """The kernel's Levenberg-Marquardt (lm_ref.lm; include/smilfit.h, smil_refine_cameras).  Returns a dict: params (10), status,
    n_accepted, n_trials, cost0, cost, g (10), lam, margin."""
    if len(p3) < MIN_POINTS:
        return dict(params=np.asarray(params10, np.float64).copy(), status=SKIPPED, n_accepted=0, n_trials=0, cost0=np.nan, cost=np.nan, g=np.zeros(10), lam=1e-3, margin=np.inf, trace=[])
    out = lm_ref.lm(lambda x: evaluate(x, p3, p2, n_params, f_scale), params10, n_params, max_steps)
    out["params"] = out["x"]
    return out


def lm_exact(params10, p3, p2, n_params=10, f_scale=5.0, max_steps=100):
    """The exact-step iteration (lm_ref.lm_exact) of a camera with at least MIN_POINTS correspondences: the dict of lm()."""
    out = lm_ref.lm_exact(lambda x: evaluate_mp(x, p3, p2, f_scale, lm_ref.DIGITS, rounded=False), lm_ref.solve_mp, params10, n_params, max_steps)
    out["params"] = out["x"]
    return out


def rotation_distance(params_a, params_b):
    """max |R_a - R_b|, max |t_a - t_b| / max |t_b|, max |k_a - k_b| / max |k_b| (k = fx, fy, cx, cy)."""
    a, b = np.asarray(params_a, np.float64), np.asarray(params_b, np.float64)
    return (float(np.abs(rodrigues(a[:3])[0] - rodrigues(b[:3])[0]).max()), float(np.abs(a[3:6] - b[3:6]).max() / np.abs(b[3:6]).max()),
            float(np.abs(a[6:] - b[6:]).max() / np.abs(b[6:]).max()))


def tight10(fx, n_params):
    """The fixture's tight solution as (C, 10) parameter rows (6 parameters: the initial intrinsics)."""
    x = fx["init_params"].copy()
    x[:, :n_params] = fx[f"p{n_params}_tight_x"]
    return x


_HP = {}


def high_precision(fx, cam):
    """(cost, g, H) of camera `cam` of the fixture at its INITIAL parameters: the 40-digit values, and numpy's own (the yardstick).
    Computed once per camera and shared."""
    if cam not in _HP:
        p3, p2 = correspondences(fx)[cam]
        _HP[cam] = (evaluate_mp(fx["init_params"][cam], p3, p2, float(fx["f_scale"])), evaluate(fx["init_params"][cam], p3, p2, 10, float(fx["f_scale"])))
    return _HP[cam]


def errors(got, exact, n_params):
    """Relative errors (cost, g, H) of an accumulation against the 40-digit one, on the n_params block."""
    g_x, H_x = block(exact[1], exact[2], n_params)
    return abs(got[0] - exact[0]) / abs(exact[0]), rel_err(got[1], g_x), rel_err(got[2], H_x)
