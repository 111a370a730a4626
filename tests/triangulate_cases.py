"""The generated case sets of the triangulation tests, shared by the CPU test of their ambiguity condition and the GPU tests: every
set is seeded, solved once by the restatement (tests/triangulate_ref.py) and cached.

n2 .. n32     C = n cameras on a ring, 1100 px focal lengths (the conditioning of real rigs), every view valid, 1 px noise, up to three
              gross outliers.  n = 2 is the plain-DLT branch, 3 the smallest RANSAC, 10 (45 pairs) and 11 (55) the two sides of the
              table switch, 32 the cap.  The problem counts run from 1 to counts that are no multiple of the four problems of a
              workgroup.
drops         12 cameras, five views dropped per problem (n = 7), minimum 3 views.
ties          4 cameras; two of them see one point and the other two another, so the pairs (a, b) and (c, d) both count 2 inliers,
              with different inliers: the lowest-index hypothesis must win.
nearpar       8 cameras in four near-parallel pairs (baseline 1e-3 of the distance), and nearpar2: one such pair alone.
"""
import functools

import numpy as np

import triangulate_ref as R

SIZES = {2: 1, 3: 7, 4: 5, 10: 6, 11: 6, 12: 9, 32: 5}
CASES = [f"n{n}" for n in SIZES] + ["drops", "ties", "nearpar", "nearpar2"]
ACCURACY_SETS = ["n2", "n4", "n12", "n32", "nearpar", "nearpar2"]


def _ties():
    P = R.ring_rig(4, 40)
    rng = np.random.default_rng(41)
    groups = [((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)), ((2, 3), (0, 1)), ((1, 2), (0, 3)), ((1, 3), (0, 2))]
    obs = np.zeros((len(groups), 1, 4, 2))
    for i, (ga, gb) in enumerate(groups):
        A = rng.uniform(-0.4, 0.4, 3)
        B = A + np.array([0.5, -0.4, 0.3]) * rng.choice([-1.0, 1.0], 3)
        for cams, X in ((ga, A), (gb, B)):
            for c in cams:
                h = P[c] @ np.append(X, 1.0)
                obs[i, 0, c] = h[:2] / h[2] + rng.normal(0.0, 0.3, 2)
    return P, obs


@functools.lru_cache(maxsize=None)
def get(name):
    kw = dict(thr=15.0, min_views=2, use_ransac=True)
    if name == "ties":
        P, obs = _ties()
    elif name == "drops":
        P = R.ring_rig(12, 12)
        obs, _ = R.make_cases(P, 6, 13, drop=5)
        kw["min_views"] = 3
    elif name == "nearpar":
        P = R.ring_rig(8, 4, baseline=1e-3)
        obs, _ = R.make_cases(P, 6, 5)
    elif name == "nearpar2":
        P = R.ring_rig(2, 4, baseline=1e-3)
        obs, _ = R.make_cases(P, 6, 6, outliers=0)
    else:
        n = int(name[1:])
        P = R.ring_rig(n, n)
        obs, _ = R.make_cases(P, SIZES[n], 100 + n, outliers=0 if n == 2 else 3)
    res = R.solve_all(P, obs, None, thr=kw["thr"], min_views=kw["min_views"], use_ransac=kw["use_ransac"])
    return dict(P=P, obs=obs, res=res, **kw)
