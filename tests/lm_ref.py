"""The Levenberg-Marquardt loop of the multi-view kernels (csrc/lm.h) in float64 numpy, once, for the restatements of the camera
refinement (refine_ref.py) and of the point refinement (refine_points_ref.py): lm().  lm_exact() applies the same rules with every
evaluation and every solve in 40 digits and only the candidates rounded to float64: the yardstick of a trajectory.  Both return a
trace, one entry per evaluation, from which prefix() reads the result of a run with a smaller max_steps."""
import numpy as np

CONVERGED, STEP_LIMIT, NONFINITE = 0, 1, 3
START, ACCEPT, REJECT, NONFINITE_COST = "start", "accept", "reject", "nonfinite"  # the decisions of a trace
DIGITS = 40
SAFE_MARGIN = 1e-9  # a decision this far from cost_new == cost_cur cannot flip between two float64 evaluations (tests/lm_cases.py)


def rel_err(x, ref):
    """max |x - ref| / max |ref|: the error of a scalar, vector or matrix in units of its largest entry."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def solve_numpy(H, g, lam, n):
    """(H + lam diag H) d = -g on the leading n block by numpy's Cholesky; None when it fails or d is not finite."""
    A = H[:n, :n] + lam * np.diag(np.diag(H[:n, :n]))
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(A)
            d = np.linalg.solve(L.T, np.linalg.solve(L, -g[:n]))
    except np.linalg.LinAlgError:
        return None
    return d if bool(np.isfinite(d).all() and np.isfinite(L).all()) else None


def solve_mp(H, g, lam, n):
    """The same system in the working precision of mpmath, factorised by rows as lm_solve does and refused by its criterion: a
    pivot that is not positive and finite (or a d that is not finite).  H and g hold mpf entries; returns [mpf] * n or None."""
    import mpmath as mp

    lam = mp.mpf(float(lam))
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            v = H[j][i]
            if i == j:
                v = v + lam * v
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            if i == j:
                if not (mp.isfinite(v) and v > 0):
                    return None
                L[i][i] = mp.sqrt(v)
            else:
                L[i][j] = v / L[j][j]
    d = [mp.mpf(0)] * n
    for i in range(n):
        v = -g[i]
        for k in range(i):
            v = v - L[i][k] * d[k]
        d[i] = v / L[i][i]
    for i in range(n - 1, -1, -1):
        v = d[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * d[k]
        d[i] = v / L[i][i]
    return d if all(mp.isfinite(v) for v in d) else None


def _margin(cost_new, cost_cur):
    """|cost_new - cost_cur| / cost_cur as a float; at cost_cur == 0 an equal cost has margin 0 and any other is infinitely far."""
    diff = abs(cost_new - cost_cur)
    if cost_cur == 0:
        return 0.0 if diff == 0 else np.inf
    return float(diff / cost_cur)


def _iterate(evaluate, solve, step_to, finite, x0, n, max_steps):
    """csrc/lm.h rule for rule.  evaluate(x) returns (cost, g, H) and solve(H, g, lam, n) a step or None, both in the arithmetic of
    the caller; step_to(cur, d) is the float64 candidate.  lambda is float64 state in every arithmetic, as in the kernel."""
    x0 = np.asarray(x0, np.float64).copy()
    out = dict(x=x0.copy(), status=STEP_LIMIT, n_accepted=0, n_trials=0, cost0=np.nan, cost=np.nan, g=np.zeros(len(x0)), lam=1e-3,
               margin=np.inf, trace=[])
    cur, cand, lam = x0.copy(), x0.copy(), 1e-3
    cost_cur, g, H = np.nan, None, None
    for step in range(max_steps):
        cost_new, g_new, H_new = evaluate(cand)
        out["n_trials"] += 1
        ok = finite(cost_new)
        entry = dict(cost=float(cost_new), decision=START, refused=False, margin=np.inf, exempt=False)
        if step == 0 and not ok:
            entry.update(decision=NONFINITE_COST, lam=lam, x=cur.copy(), cost_cur=float(cost_new), n_accepted=0, done=True)
            out["trace"].append(entry)
            out.update(status=NONFINITE, cost0=float(cost_new), cost=float(cost_new))
            return out
        done = False
        if step > 0:
            # the candidate is the current point bit for bit (after a refused solve, or a step that rounds to zero): both kernels are
            # bit-reproducible, so the evaluation repeats the current cost and the rejection cannot flip
            entry["exempt"] = bool(np.array_equal(cand.view(np.int64), cur.view(np.int64)))
            if ok:
                entry["margin"] = _margin(cost_new, cost_cur)
                if not entry["exempt"]:
                    out["margin"] = min(out["margin"], entry["margin"])
        if step == 0 or (ok and cost_new < cost_cur):
            if step == 0:
                out["cost0"] = float(cost_new)
            else:
                entry["decision"] = ACCEPT
                out["n_accepted"] += 1
                lam = max(lam / 10.0, 1e-12)
                done = bool(cost_cur - cost_new < 1e-12 * cost_cur)
            cur, g, H, cost_cur = cand.copy(), g_new, H_new, cost_new
        else:
            entry["decision"] = REJECT if ok else NONFINITE_COST
            lam *= 10.0
        done = done or lam > 1e12
        if not done:
            d = solve(H, g, lam, n)
            cand = cur.copy()
            if d is not None:
                cand[:n] = step_to(cur[:n], d)
            else:
                entry["refused"] = True
                lam *= 10.0
                done = lam > 1e12
        entry.update(lam=lam, x=cur.copy(), cost_cur=float(cost_cur), g_cur=np.array([float(v) for v in g]), n_accepted=out["n_accepted"],
                     done=bool(done))
        out["trace"].append(entry)
        if done:
            out["status"] = CONVERGED
            break
    out.update(x=cur, cost=float(cost_cur), g=np.array([float(v) for v in g]), lam=lam)
    return out


def lm(evaluate, x0, n_free, max_steps):
    """csrc/lm.h rule for rule from x0, whose first n_free entries move; evaluate(x) returns (cost, g, H) in float64.  Returns a dict: x,
    status, n_accepted, n_trials, cost0, cost, g (zeros when the start has no finite cost), lam, margin: the smallest
    |cost_new - cost_cur| / cost_cur over the accept / reject decisions that are not exempt (how far the closest decision is from going
    the other way), and trace: one dict per evaluation with cost (the cost evaluated), decision (START, ACCEPT, REJECT or
    NONFINITE_COST), refused (lm_solve gave no step afterwards), lam, x, cost_cur, n_accepted (all after the step), done, margin (of
    this decision) and exempt (the evaluation was of the current point bit for bit: it cannot flip and has no margin to keep)."""
    return _iterate(evaluate, solve_numpy, lambda cur, d: cur + d, lambda c: bool(np.isfinite(c)), x0, n_free, max_steps)


def lm_exact(evaluate_exact, solve, x0, n_free, max_steps, digits=DIGITS):
    """The exact-step iteration: lm()'s rules with evaluate_exact(x) -> (cost, g, H) as unrounded mpf values and solve (solve_mp) in
    `digits` digits; only each candidate is rounded to float64.  Returns what lm returns, its costs and g rounded at the end."""
    import mpmath as mp

    def evaluate(x):
        try:
            return evaluate_exact(x)
        except ZeroDivisionError:
            return mp.nan, None, None

    def step_to(cur, d):
        return np.array([float(mp.mpf(float(c)) + v) for c, v in zip(cur, d)])

    with mp.workprec(int(digits * 3.33) + 8):
        return _iterate(evaluate, solve, step_to, lambda c: bool(mp.isfinite(c)), x0, n_free, max_steps)


def prefix(out, k):
    """What a run with max_steps = k returns, read from the trace of a run with a larger max_steps: dict of x, status, n_accepted,
    n_trials, cost0, cost, g."""
    t = out["trace"]
    if k >= len(t):
        return dict(x=out["x"], status=out["status"], n_accepted=out["n_accepted"], n_trials=out["n_trials"], cost0=out["cost0"], cost=out["cost"],
                    g=out["g"])
    e = t[k - 1]
    return dict(x=e["x"], status=CONVERGED if e["done"] else STEP_LIMIT, n_accepted=e["n_accepted"], n_trials=k, cost0=out["cost0"], cost=e["cost_cur"],
                g=e["g_cur"])


def safe_prefix(out, margin=SAFE_MARGIN):
    """The number of leading evaluations all of whose non-exempt decisions have a margin of at least `margin`."""
    k = 0
    for e in out["trace"]:
        if e["decision"] in (ACCEPT, REJECT) and not e["exempt"] and e["margin"] < margin:
            break
        k += 1
    return k


def decisions(out):
    """The decisions of a trace as a string: S start, A accept, R reject, N non-finite; lower case where lm_solve refused afterwards."""
    s = "".join({START: "S", ACCEPT: "A", REJECT: "R", NONFINITE_COST: "N"}[e["decision"]] for e in out["trace"])
    return "".join(c.lower() if e["refused"] else c for c, e in zip(s, out["trace"]))
