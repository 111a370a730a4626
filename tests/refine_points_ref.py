"""float64 numpy restatement of the point refinement (csrc/refine_points.hip, an extension without a reference counterpart) for the
CPU and GPU tests: one accumulation (cost, g, H of scipy's soft_l1 on every scalar reprojection residual of a point's views, analytic
Jacobian), the kernel's exact Levenberg-Marquardt rules one problem at a time, and a 40-digit mpmath evaluation of the accumulation."""
import os

import numpy as np

import lm_ref
from lm_ref import rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONVERGED, STEP_LIMIT, FEW_VIEWS, NONFINITE = 0, 1, 2, 3
GROUPS = ("ring12", "v2", "v3", "v12", "v32", "par2")


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "refine_points_ref.npz")))


def group(fx, g):
    """P (C,3,4), obs (n,1,C,2), mask (n,1) uint32, xyz0 (n,1,3) of one group of the fixture."""
    return fx[g + "_P"], fx[g + "_obs"], fx[g + "_mask"], fx[g + "_xyz0"]


def views_of(mask, C):
    return np.flatnonzero([(int(mask) >> c) & 1 for c in range(C)])


def jacobian(P, X):
    """The projections (n, 2) and Jacobian rows (n, 2, 3) of the views P (n, 3, 4) at X: (P[k,:3] - (h_k / h2) P[2,:3]) / h2."""
    with np.errstate(all="ignore"):
        h = P[:, :, :3] @ X + P[:, :, 3]
        q = h[:, :2] / h[:, 2:3]
        J = (P[:, :2, :3] - q[:, :, None] * P[:, 2:3, :3]) * (1.0 / h[:, 2])[:, None, None]
    return q, J


def evaluate(P, obs, mask, X, f_scale=5.0):
    """cost, g (3), H (3, 3) of one problem in float64: P (C,3,4), obs (C,2), the views of the bits of mask.  Views outside the mask
    are never touched; no view gives zeros."""
    v = views_of(mask, len(P))
    q, J = jacobian(P[v], np.asarray(X, np.float64))
    with np.errstate(all="ignore"):
        f = q - obs[v]
        z = (f / f_scale) ** 2
        h = np.sqrt(1.0 + z)
        cost = 0.5 * f_scale ** 2 * float(np.sum(2.0 * z / (h + 1.0)))
        w = 1.0 / h
        g = np.einsum("nki,nk->i", J, w * f)
        H = np.triu(np.einsum("nki,nk,nkj->ij", J, w, J))  # the upper triangle, mirrored: what the kernel sums
    return cost, g, H + np.triu(H, 1).T


def evaluate_mp(P, obs, mask, X, f_scale=5.0, digits=40, rounded=True):
    """The same accumulation in `digits`-digit arithmetic, rounded to float64.  rounded=False: the unrounded mpf values, cost, g as a
    list and H as a list of rows (for lm_ref.lm_exact)."""
    import mpmath as mp

    with mp.workprec(int(digits * 3.33) + 8):
        fs = mp.mpf(float(f_scale))
        Xm = [mp.mpf(float(x)) for x in X]
        cost, g, H = mp.mpf(0), [mp.mpf(0)] * 3, [[mp.mpf(0)] * 3 for _ in range(3)]
        for c in views_of(mask, len(P)):
            Pm = [[mp.mpf(float(P[c, i, j])) for j in range(4)] for i in range(3)]
            h = [Pm[i][0] * Xm[0] + Pm[i][1] * Xm[1] + Pm[i][2] * Xm[2] + Pm[i][3] for i in range(3)]
            for k in range(2):
                q = h[k] / h[2]
                f = q - mp.mpf(float(obs[c, k]))
                J = [(Pm[k][j] - q * Pm[2][j]) / h[2] for j in range(3)]
                hh = mp.sqrt(1 + (f / fs) ** 2)
                cost += 2 * (hh - 1)
                w = 1 / hh
                for i in range(3):
                    g[i] += J[i] * w * f
                    for j in range(3):
                        H[i][j] += w * J[i] * J[j]
        if not rounded:
            return fs * fs * cost / 2, g, H
        return float(fs * fs * cost / 2), np.array([float(x) for x in g]), np.array([[float(x) for x in row] for row in H])


def errors(got, exact):
    return tuple(rel_err(a, b) for a, b in zip(got, exact))


def lm(P, obs, mask, xyz0, f_scale=5.0, max_steps=50):
    """The kernel's Levenberg-Marquardt (lm_ref.lm; include/smilfit.h, smil_refine_points).  Returns a dict: xyz, status, n_accepted,
    n_trials, cost0, cost, and margin: the smallest |cost_new - cost_cur| / cost_cur over its accept / reject decisions (how far the
    closest decision is from going the other way)."""
    if len(views_of(mask, len(P))) < 2:
        return dict(xyz=np.asarray(xyz0, np.float64).copy(), status=FEW_VIEWS, n_accepted=0, n_trials=0, cost0=np.nan, cost=np.nan, margin=np.inf, trace=[])
    out = lm_ref.lm(lambda x: evaluate(P, obs, mask, x, f_scale), xyz0, 3, max_steps)
    return dict(xyz=out["x"], **{k: out[k] for k in ("x", "g", "status", "n_accepted", "n_trials", "cost0", "cost", "margin", "trace")})


def lm_exact(P, obs, mask, xyz0, f_scale=5.0, max_steps=50):
    """The exact-step iteration (lm_ref.lm_exact) of a problem with at least two views: the dict of lm()."""
    out = lm_ref.lm_exact(lambda x: evaluate_mp(P, obs, mask, x, f_scale, lm_ref.DIGITS, rounded=False), lm_ref.solve_mp, xyz0, 3, max_steps)
    return dict(xyz=out["x"], **{k: out[k] for k in ("x", "g", "status", "n_accepted", "n_trials", "cost0", "cost", "margin", "trace")})


def distance(a, b):
    """max |a - b| / max |b|: the distance of two points relative to |X|."""
    return rel_err(a, b)


_LM, _HP = {}, {}


def lm_group(fx, g):
    """lm() of every problem of a group: computed once and shared."""
    if g not in _LM:
        P, obs, mask, xyz0 = group(fx, g)
        _LM[g] = [lm(P, obs[i, 0], mask[i, 0], xyz0[i, 0], float(fx["f_scale"])) for i in range(len(obs))]
    return _LM[g]


def high_precision(key, P, obs, mask, X, f_scale=5.0):
    """(the 40-digit cost, g, H; numpy's own) of one problem, computed once per key and shared."""
    if key not in _HP:
        _HP[key] = (evaluate_mp(P, obs, mask, X, f_scale), evaluate(P, obs, mask, X, f_scale))
    return _HP[key]
