"""The Levenberg-Marquardt loop of the multi-view kernels (csrc/lm.h) in float64 numpy, once, for the restatements of the camera
refinement (refine_ref.py) and of the point refinement (refine_points_ref.py)."""
import numpy as np

CONVERGED, STEP_LIMIT, NONFINITE = 0, 1, 3


def rel_err(x, ref):
    """max |x - ref| / max |ref|: the error of a scalar, vector or matrix in units of its largest entry."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def lm(evaluate, x0, n_free, max_steps):
    """csrc/lm.h rule for rule from x0, whose first n_free entries move; evaluate(x) returns (cost, g, H).  Returns a dict: x, status,
    n_accepted, n_trials, cost0, cost, g (zeros when the start has no finite cost), lam, and margin: the smallest
    |cost_new - cost_cur| / cost_cur over the accept / reject decisions (how far the closest decision is from going the other way)."""
    x0, n = np.asarray(x0, np.float64).copy(), n_free
    out = dict(x=x0.copy(), status=STEP_LIMIT, n_accepted=0, n_trials=0, cost0=np.nan, cost=np.nan, g=np.zeros(len(x0)), lam=1e-3,
               margin=np.inf)
    cur, cand, lam = x0.copy(), x0.copy(), 1e-3
    cost_cur, g, H = np.nan, None, None
    for step in range(max_steps):
        cost_new, g_new, H_new = evaluate(cand)
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
            A = H[:n, :n] + lam * np.diag(np.diag(H[:n, :n]))
            try:
                with np.errstate(all="ignore"):
                    L = np.linalg.cholesky(A)
                    d = np.linalg.solve(L.T, np.linalg.solve(L, -g[:n]))
                ok = bool(np.isfinite(d).all() and np.isfinite(L).all())
            except np.linalg.LinAlgError:
                ok = False
            cand = cur.copy()
            if ok:
                cand[:n] = cur[:n] + d
            else:
                lam *= 10.0
                done = lam > 1e12
        if done:
            out["status"] = CONVERGED
            break
    out.update(x=cur, cost=cost_cur, g=g, lam=lam)
    return out
