"""Writes tests/golden/refine_points_ref.npz: scipy's least_squares on the reprojection residuals of single points, the yardstick of the
point refinement (csrc/refine_points.hip).  The reference has no such function, so nothing of it is run here.  Needs scipy.

    python tests/golden/make_refine_points_fixture.py

Per problem ``least_squares(residuals, xyz0, method="trf", loss="soft_l1", f_scale=5)`` twice: at scipy's defaults, and TIGHT
(ftol = xtol = gtol = 1e-15) started from the default result.  Groups of problems, each with its own cameras:

* ``ring12``: the 12 ring cameras and the observations of tests/golden/triangulate_ref.npz (read, not modified); per triangulated
  problem the views of the final system and the point of the pair RANSAC (tests/triangulate_ref.py, checked here against the recorded
  tracks of the reference).  Dropped views keep their NaN or (0, 0) observation, gross outliers outside the mask stay where they are.
* ``v2``, ``v3``, ``v12``, ``v32``: seeded rings of 2, 3, 12 and 32 cameras, six points each, 1 px noise, started from the DLT point of
  the mask's views.  In v12 and v32 some problems drop views, the lowest and the highest bit among them (their observations are NaN).
  Problem 0 of v3, v12 and v32 has ONE gross outlier of 10 - 14 px left inside the mask (what a 15 px RANSAC threshold lets through);
  in v12 the other views of that problem carry 0.2 px noise, so that the pull of the outlier is what the start suffers from.
* ``par2``: one near-parallel pair (baseline 2 % of the distance), four points.

A soft_l1 cost with outliers can have more than one minimum.  Only problems where scipy-default, scipy-tight and the numpy restatement
of the kernel's rules (tests/refine_points_ref.py) end at the same minimum, points within 1e-5 (relative) of one another, are kept;
at least 95 % of the generated problems must survive.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refine_points_ref as R  # noqa: E402
import triangulate_ref as T  # noqa: E402

SEED, F_SCALE, SAME = 52, 5.0, 1e-5


def mask_of(views):
    return np.uint32(sum(1 << int(c) for c in views))


def generated(C, rng, n, baseline=None, drops=(), outlier=None, quiet=None):
    """n problems through a ring of C cameras: obs (n,1,C,2), mask (n,1), xyz0 (n,1,3), X_true (n,3)."""
    P = T.ring_rig(C, int(rng.integers(1 << 30)), baseline=baseline)
    X = rng.uniform(-0.5, 0.5, (n, 3))
    h = np.einsum("cij,nj->nci", P, np.concatenate([X, np.ones((n, 1))], axis=1))
    obs = h[..., :2] / h[..., 2:3] + rng.normal(0.0, 1.0, (n, C, 2))
    if quiet is not None:
        obs[quiet] = (h[..., :2] / h[..., 2:3])[quiet] + rng.normal(0.0, 0.2, (C, 2))
    if outlier is not None:
        i, c = outlier
        ang = rng.uniform(0.0, 2.0 * np.pi)
        obs[i, c] += rng.uniform(10.0, 14.0) * np.array([np.cos(ang), np.sin(ang)])
    mask, xyz0 = np.zeros((n, 1), np.uint32), np.zeros((n, 1, 3))
    for i in range(n):
        views = np.setdiff1d(np.arange(C), drops[i] if i < len(drops) else [])
        obs[i, np.setdiff1d(np.arange(C), views)] = np.nan
        mask[i, 0], xyz0[i, 0] = mask_of(views), T.dlt(P[views], obs[i, views])
    return P, obs[:, None], mask, xyz0, X


def ring12():
    fx = T.fixture()
    P, obs, scores = T.fixture_arrays(fx, 12)
    res = T.solve_all(P, obs, scores, conf=0.3, min_views=2, thr=15.0, use_ransac=True)
    tracks = fx["all_c12_ransac_mv2_tracks"][:, 0]
    keep = [(f, k) for f in range(obs.shape[0]) for k in range(obs.shape[1]) if res[f, k]["status"] == 0]
    for f, k in keep:
        assert np.allclose(res[f, k]["xyz"], tracks[f, k], rtol=1e-9, atol=1e-12), (f, k)
    o = np.stack([obs[f, k] for f, k in keep])[:, None]
    m = np.asarray([[res[f, k]["cam_mask"]] for f, k in keep], np.uint32)
    x0 = np.stack([res[f, k]["xyz"] for f, k in keep])[:, None]
    return P, o, m, x0, np.stack([fx["X_true"][f, k] for f, k in keep])


def solve(P, obs, mask, xyz0):
    from scipy.optimize import least_squares

    v = R.views_of(mask, len(P))

    def residuals(X):
        h = P[v, :, :3] @ X + P[v, :, 3]
        return (h[:, :2] / h[:, 2:3] - obs[v]).ravel()

    kw = dict(method="trf", loss="soft_l1", f_scale=F_SCALE)
    default = least_squares(residuals, xyz0, **kw)
    tight = least_squares(residuals, default.x, ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000, **kw)
    return default, tight


def main():
    rng = np.random.default_rng(SEED)
    groups = dict(ring12=ring12(),
                  v2=generated(2, rng, 6),
                  v3=generated(3, rng, 6, outlier=(0, 1)),
                  v12=generated(12, rng, 6, drops=([], [0], [11], [0, 11], [3, 4, 5, 6, 7]), outlier=(0, 7), quiet=0),
                  v32=generated(32, rng, 6, drops=([], [0], [31], [0, 31], list(range(1, 31, 2))), outlier=(0, 20)),
                  par2=generated(2, rng, 4, baseline=0.02))
    assert tuple(groups) == R.GROUPS
    out = dict(f_scale=np.float64(F_SCALE), outlier_cases=np.asarray(["v3", "v12", "v32"]))
    total = kept = 0
    for name, (P, obs, mask, xyz0, X_true) in groups.items():
        rows, keep = [], []
        for i in range(len(obs)):
            default, tight = solve(P, obs[i, 0], mask[i, 0], xyz0[i, 0])
            own = R.lm(P, obs[i, 0], mask[i, 0], xyz0[i, 0], F_SCALE)
            d = (R.distance(default.x, tight.x), R.distance(own["xyz"], tight.x), R.distance(own["xyz"], default.x))
            same = max(d) <= SAME
            print(f"{name} {i}: views {len(R.views_of(mask[i, 0], len(P)))} nfev {default.nfev}+{tight.nfev} trials {own['n_trials']} "
                  f"cost dlt {own['cost0']:.6f} default {default.cost:.9f} tight {tight.cost:.9f} own {own['cost']:.9f} "
                  f"distances {d[0]:.1e} {d[1]:.1e} {d[2]:.1e} {'' if same else 'DROPPED'}")
            keep.append(same)
            rows.append((default.x, default.cost, tight.x, tight.cost))
        if name in out["outlier_cases"]:
            assert keep[0], name  # the outlier problem of the group leads it
        k = np.flatnonzero(keep)
        total, kept = total + len(keep), kept + len(k)
        out[name + "_P"], out[name + "_obs"], out[name + "_mask"], out[name + "_xyz0"] = P, obs[k], mask[k], xyz0[k]
        out[name + "_X_true"] = X_true[k]
        out[name + "_scipy_x"], out[name + "_scipy_cost"] = np.stack([rows[i][0] for i in k]), np.asarray([rows[i][1] for i in k])
        out[name + "_tight_x"], out[name + "_tight_cost"] = np.stack([rows[i][2] for i in k]), np.asarray([rows[i][3] for i in k])
    out["generated"], out["kept"] = np.int64(total), np.int64(kept)
    print(f"kept {kept} of {total}")
    assert kept >= 0.95 * total
    path = os.path.join(HERE, "refine_points_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
