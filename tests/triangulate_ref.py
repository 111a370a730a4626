"""float64 numpy restatement of the triangulation semantics (reference smal_fitter/sleap_data/triangulate_3d_points.py :156-301,
:830-978) for the CPU and GPU tests: the view filter, the plain DLT, the pair RANSAC with the lowest-index-of-the-maximum selection and
EVERY hypothesis's per-view errors (so tests can see the margins to the threshold), the five-round undistortion with its forward
model, and a 40-digit mpmath evaluation of a DLT system."""
import itertools
import os

import numpy as np

MAX_VIEWS, MAX_HYP = 32, 50
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "triangulate_ref.npz")))


def pair_list(n, max_hypotheses=MAX_HYP):
    """The hypotheses of n valid views (:240-245)."""
    pairs = list(itertools.combinations(range(n), 2))
    if len(pairs) > max_hypotheses:
        rng = np.random.default_rng(42)
        pairs = [pairs[i] for i in rng.choice(len(pairs), max_hypotheses, replace=False)]
    return pairs


def dlt_rows(Ps, pts):
    """(2n, 4): rows x P[2] - P[0], y P[2] - P[1] of every view (:168-172)."""
    Ps, pts = np.asarray(Ps, np.float64), np.asarray(pts, np.float64)
    A = np.empty((2 * len(Ps), 4))
    A[0::2] = pts[:, 0:1] * Ps[:, 2] - Ps[:, 0]
    A[1::2] = pts[:, 1:2] * Ps[:, 2] - Ps[:, 1]
    return A


def dlt(Ps, pts):
    X = np.linalg.svd(dlt_rows(Ps, pts))[2][-1]
    with np.errstate(all="ignore"):
        return X[:3] / X[3]


def reproj_errors(Ps, X, pts):
    with np.errstate(all="ignore"):
        proj = np.asarray(Ps, np.float64) @ np.append(X, 1.0)
        return np.linalg.norm(proj[:, :2] / proj[:, 2:3] - pts, axis=1)


def valid_views(obs, scores, conf):
    """(C,) bool: the views :915-920 keep.  obs (C, 2), scores (C,) or None."""
    ok = ~np.isnan(obs).any(axis=1) & ~((obs[:, 0] == 0) & (obs[:, 1] == 0))
    if scores is not None:
        with np.errstate(invalid="ignore"):
            ok &= ~(~np.isnan(scores) & (scores < conf))
    return ok


def undistort5(pts, K, dist):
    """cv2.undistortPoints(pts, K, dist, P=K) as documented: five rounds of x <- (x0 - tangential(x)) / radial(x)."""
    k1, k2, p1, p2, k3 = dist
    x0, y0 = (pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    w = K[2, 0] * x + K[2, 1] * y + K[2, 2]
    return np.stack([(K[0, 0] * x + K[0, 1] * y + K[0, 2]) / w, (K[1, 0] * x + K[1, 1] * y + K[1, 2]) / w], axis=1)


def distort(pts, K, dist):
    """The forward model the recurrence inverts: ideal pixels -> distorted pixels (zero skew)."""
    k1, k2, p1, p2, k3 = dist
    x, y = (pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1]
    r2 = x * x + y * y
    radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)


def solve(P, obs, scores=None, conf=0.3, min_views=2, thr=15.0, use_ransac=True, K=None, dist=None, keep_all=False):
    """One problem.  P (C, 3, 4), obs (C, 2), scores (C,) or None.  Returns a dict: status (0 / 1 insufficient views / 2 RANSAC
    failed), xyz, views_used, valid (C,) bool, pts (C, 2) the points after undistortion, cam_mask (bits of the cameras of the final
    system), final (camera indices of the final system), hyp_err ((H, n) per-view errors of every hypothesis, or None), hyp_count,
    winner, mean_err, view_err (C,)."""
    P, obs = np.asarray(P, np.float64), np.asarray(obs, np.float64)
    C = len(P)
    valid = np.ones(C, bool) if keep_all else valid_views(obs, scores, conf)
    pts = obs.copy()
    if K is not None:
        for c in np.flatnonzero(valid):
            if not np.allclose(dist[c], 0):
                pts[c] = undistort5(pts[c:c + 1], K[c], dist[c])[0]
    cams = np.flatnonzero(valid)
    n = len(cams)
    out = dict(status=0, xyz=np.full(3, np.nan), views_used=0, valid=valid, pts=pts, cam_mask=0, final=cams[:0], hyp_err=None,
               hyp_count=None, winner=-1, mean_err=np.nan, view_err=np.full(C, np.nan), n=n)
    if n < min_views:
        out["status"] = 1
        return out
    Ps, p2 = P[cams], pts[cams]
    final = np.arange(n)
    if use_ransac and n >= 3:
        pairs = pair_list(n)
        errs = np.stack([reproj_errors(Ps, dlt(Ps[[i, j]], p2[[i, j]]), p2) for i, j in pairs])
        with np.errstate(invalid="ignore"):
            inl = errs < thr
        count = inl.sum(axis=1)
        winner = int(np.argmax(count))  # the first of the largest: the lowest-index hypothesis with the maximum count
        out.update(hyp_err=errs, hyp_count=count, winner=winner)
        if count[winner] < min_views:
            out["status"] = 2
            return out
        final = np.flatnonzero(inl[winner])
    X = dlt(Ps[final], p2[final])
    e = reproj_errors(Ps, X, p2)
    out.update(xyz=X, views_used=len(final), final=cams[final], cam_mask=int(sum(1 << int(c) for c in cams[final])), mean_err=float(e.mean()))
    out["view_err"][cams] = e
    return out


def solve_all(P, obs, scores=None, **kw):
    """Every problem of obs (N, Kp, C, 2): a (N, Kp) object array of solve() dicts."""
    N, Kp = obs.shape[:2]
    res = np.empty((N, Kp), object)
    for f in range(N):
        for k in range(Kp):
            res[f, k] = solve(P, obs[f, k], None if scores is None else scores[f, k], **kw)
    return res


def field(res, name, dtype=None):
    return np.asarray([[r[name] for r in row] for row in res], dtype)


def ambiguous(res, thr=15.0, tol=1e-6):
    """The number of problems in which some hypothesis has a view within tol px of the threshold."""
    return sum(1 for r in res.ravel() if r["hyp_err"] is not None and bool((np.abs(r["hyp_err"] - thr) <= tol).any()))


def final_system(P, r):
    """The rows of the final DLT system of a solved problem."""
    return dlt_rows(P[r["final"]], r["pts"][r["final"]])


def dlt_mp(A, digits=40):
    """X[:3] / X[3] of the smallest right singular vector of A in `digits`-digit arithmetic, rounded to float64."""
    import mpmath

    with mpmath.workprec(int(digits * 3.33) + 8):
        _, S, V = mpmath.svd_r(mpmath.matrix(A.tolist()), full_matrices=False, compute_uv=True)
        row = min(range(len(S)), key=lambda i: S[i])
        X = [V[row, j] for j in range(4)]
        return np.asarray([float(X[j] / X[3]) for j in range(3)])


def rel_err(X, X_mp):
    return float(np.abs(X - X_mp).max() / np.abs(X_mp).max())


def fixture_arrays(fx, ncam):
    """(P, obs (N, Kp, C, 2), scores (N, Kp, C)) of the fixture's first ncam cameras as triangulate_all hands them to the kernel:
    frames beyond a camera's own count are NaN."""
    coords, scores = fx["coords"][:ncam].copy(), fx["scores"][:ncam].copy()
    for c in range(ncam):
        coords[c, fx["frames_of"][c]:] = np.nan
        scores[c, fx["frames_of"][c]:] = np.nan
    return fx["P"][:ncam], np.ascontiguousarray(coords.transpose(1, 2, 0, 3)), np.ascontiguousarray(scores.transpose(1, 2, 0))


def fixture_calibration(fx, ncam):
    """The cameras / all_coords / all_scores dicts of triangulate_all."""
    names = [f"cam{c:02d}" for c in range(ncam)]
    cams = {n: dict(K=fx["K"][c], dist=np.zeros(5), R=fx["R"][c], t=fx["t"][c]) for c, n in enumerate(names)}
    coords = {n: fx["coords"][c, :fx["frames_of"][c]] for c, n in enumerate(names)}
    scores = {n: fx["scores"][c, :fx["frames_of"][c]] for c, n in enumerate(names)}
    return cams, coords, scores


def ring_rig(C, seed, focal=1100.0, radius=4.0, baseline=None):
    """C look-at projection matrices (C, 3, 4) on a ring.  ``baseline``: the cameras come in near-parallel neighbours, every odd one
    `baseline` x radius beside the even one before it."""
    rng = np.random.default_rng(seed)
    P = []
    for c in range(C):
        az = 2.0 * np.pi * (c - (c % 2 if baseline else 0)) / C + (0.0 if baseline else rng.uniform(-0.05, 0.05))
        eye = np.array([radius * np.cos(az), radius * np.sin(az), 1.5 + 0.5 * (c % 3 if not baseline else 0)])
        if baseline and c % 2:
            eye = eye + baseline * radius * np.array([-np.sin(az), np.cos(az), 0.0])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        K = np.array([[focal, 0.0, 0.58 * focal], [0.0, focal * 1.01, 0.47 * focal], [0.0, 0.0, 1.0]])
        P.append(K @ np.hstack([R, (-R @ eye)[:, None]]))
    return np.stack(P)


def make_cases(P, n_problems, seed, noise=1.0, outliers=3, outlier_px=(120.0, 400.0), drop=0):
    """Seeded observations (n_problems, 1, C, 2) of random points through P, pixel noise `noise` (in units of focal / 1100 px), up to
    `outliers` gross outliers and exactly `drop` NaN views per problem."""
    rng = np.random.default_rng(seed)
    C = len(P)
    scale = abs(P[0, 0, 0]) / 1100.0 if abs(P[0, 0, 0]) > 1e-9 else 1.0
    scale = max(scale, np.linalg.norm(P[0, 0, :3]) / 1100.0)
    X = rng.uniform(-0.5, 0.5, (n_problems, 3))
    proj = np.einsum("cij,nj->nci", P, np.concatenate([X, np.ones((n_problems, 1))], axis=1))
    obs = proj[..., :2] / proj[..., 2:3] + noise * scale * rng.normal(0.0, 1.0, (n_problems, C, 2))
    for i in range(n_problems):
        for c in rng.permutation(C)[:rng.integers(0, outliers + 1)]:
            ang = rng.uniform(0.0, 2.0 * np.pi)
            obs[i, c] += scale * rng.uniform(*outlier_px) * np.array([np.cos(ang), np.sin(ang)])
        obs[i, rng.permutation(C)[:drop]] = np.nan
    return obs[:, None], X
