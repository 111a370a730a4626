"""float64 numpy restatement of the point refinement (csrc/refine_points.hip, an extension without a reference counterpart) for the
CPU and GPU tests: one accumulation (cost, g, H of scipy's soft_l1 on every scalar reprojection residual of a point's views, analytic
Jacobian), the kernel's exact Levenberg-Marquardt rules one problem at a time, and a 40-digit mpmath evaluation of the accumulation."""
import os

import numpy as np

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


def evaluate_mp(P, obs, mask, X, f_scale=5.0, digits=40):
    """The same accumulation in `digits`-digit arithmetic, rounded to float64."""
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
        return float(fs * fs * cost / 2), np.array([float(x) for x in g]), np.array([[float(x) for x in row] for row in H])


def rel_err(x, ref):
    """max |x - ref| / max |ref|: the error of a scalar, vector or matrix in units of its largest entry."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def errors(got, exact):
    return tuple(rel_err(a, b) for a, b in zip(got, exact))


def lm(P, obs, mask, xyz0, f_scale=5.0, max_steps=50):
    """The kernel's Levenberg-Marquardt, rule for rule (include/smilfit.h, smil_refine_points).  Returns a dict: xyz, status,
    n_accepted, n_trials, cost0, cost, and margin: the smallest |cost_new - cost_cur| / cost_cur over its accept / reject decisions
    (how far the closest decision is from going the other way)."""
    x0 = np.asarray(xyz0, np.float64).copy()
    out = dict(xyz=x0.copy(), status=STEP_LIMIT, n_accepted=0, n_trials=0, cost0=np.nan, cost=np.nan, margin=np.inf)
    if len(views_of(mask, len(P))) < 2:
        out["status"] = FEW_VIEWS
        return out
    cur, cand, lam = x0.copy(), x0.copy(), 1e-3
    cost_cur, g, H = np.nan, None, None
    for step in range(max_steps):
        cost_new, g_new, H_new = evaluate(P, obs, mask, cand, f_scale)
        out["n_trials"] += 1
        done = False
        if step == 0 and not np.isfinite(cost_new):
            out.update(status=NONFINITE, cost0=cost_new, cost=cost_new)
            return out
        if step > 0 and np.isfinite(cost_new):
            out["margin"] = min(out["margin"], abs(cost_new - cost_cur) / cost_cur)
        if step == 0 or (np.isfinite(cost_new) and cost_new < cost_cur):
            if step == 0:
                out["cost0"] = cost_new
            else:
                out["n_accepted"] += 1
                lam = max(lam / 10.0, 1e-12)
                done = cost_cur - cost_new < 1e-12 * cost_cur
            cur, g, H, cost_cur = cand.copy(), g_new, H_new, cost_new
        else:
            lam *= 10.0
        done = done or lam > 1e12
        if not done:
            A = H + lam * np.diag(np.diag(H))
            try:
                with np.errstate(all="ignore"):
                    L = np.linalg.cholesky(A)
                    d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
                ok = bool(np.isfinite(d).all() and np.isfinite(L).all())
            except np.linalg.LinAlgError:
                ok = False
            cand = cur.copy()
            if ok:
                cand = cur + d
            else:
                lam *= 10.0
                done = lam > 1e12
        if done:
            out["status"] = CONVERGED
            break
    out.update(xyz=cur, cost=cost_cur)
    return out


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
