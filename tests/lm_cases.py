"""Small seeded problems that together take every path of csrc/lm.h, for tests/test_lm_paths_cpu.py (which proves it on the
restatement) and tests/test_gpu_lm_paths.py (which holds both kernels to it).  Nothing is read from a file.

Points.  All point problems live on ONE rig of 32 projection matrices and differ in their view mask, observations and start, so
that they can share a launch and a problem alone has the lanes it has inside a batch.  Views 0-2: three narrow-baseline pinhole
cameras around (3, 0, 0.5) that look at the origin; views 3-5: the same kind with column 2 zeroed (J[:, 2] == 0 exactly); views 6-8:
P = [[64, 0, 0, 64 tx], [0, 64, 0, 64 ty], [0, 0, 1, 0]], whose projections of (1, 2, 4) are exact in float64; views 9-31: a ring.

Cameras.  24 correspondences in [-1, 1]^3 each (300 for `many`), so a launch of them has one accumulation workgroup per camera and a
camera alone gives the bits it gives inside a batch.

A case names the path it exists for (`path`, checked by the CPU test against the restatement's trace) and the least safe prefix it
must have (`min_safe`).  The safe prefix of a run is the number of leading evaluations all of whose non-exempt decisions have a
relative cost margin >= 1e-9: the existing kernel tests pin a GPU cost to max(4 x numpy's error, 2^-45) of its value, numpy's error
is of the order 1e-15, so such a decision is more than 1e4 cost errors away from going the other way on the GPU."""
import numpy as np

import lm_ref
import refine_points_ref as RP
import refine_ref as RC

F_SCALE = 5.0
POINT_STEPS, CAMERA_STEPS = 50, 100


# ---- the point rig ----
def _look_at(centre, target, focal, cx, cy):
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]]) @ np.hstack([R, (-R @ centre)[:, None]])


def _rig():
    P = np.zeros((32, 3, 4))
    for i, dy in enumerate((-0.25, 0.0, 0.25)):
        P[i] = _look_at(np.array([3.0, dy, 0.5 + 0.1 * i]), np.zeros(3), 800.0, 320.0, 240.0)
        P[3 + i] = _look_at(np.array([3.0, 4.0 * dy, 0.5 + 0.4 * i]), np.zeros(3), 800.0, 320.0, 240.0)
        P[3 + i][:, 2] = 0.0
    for i, (tx, ty) in enumerate(((0.0, 0.0), (2.0, 0.0), (0.0, 2.0))):
        P[6 + i] = [[64.0, 0.0, 0.0, 64.0 * tx], [0.0, 64.0, 0.0, 64.0 * ty], [0.0, 0.0, 1.0, 0.0]]
    for i in range(23):
        a = 2.0 * np.pi * i / 23
        P[9 + i] = _look_at(np.array([4.0 * np.cos(a), 4.0 * np.sin(a), 1.0 + 0.5 * np.sin(3.0 * a)]), np.zeros(3), 700.0, 320.0, 240.0)
    return P


POINT_P = _rig()


def _project(views, X):
    h = POINT_P[views, :, :3] @ X + POINT_P[views, :, 3]
    return h[:, :2] / h[:, 2:3]


def _point(name, path, min_safe, views, X_true, start, noise, seed, outlier=None):
    views = np.asarray(views)
    obs = np.full((32, 2), np.nan)  # what a view outside the mask holds is never read
    obs[views] = _project(views, np.asarray(X_true, np.float64))
    if noise:
        obs[views] += np.random.default_rng(seed).normal(0.0, noise, (len(views), 2))
    if outlier is not None:
        obs[outlier] += 300.0
    return dict(name=name, path=path, min_safe=min_safe, mask=np.uint32(sum(1 << int(v) for v in views)), obs=obs,
                xyz0=np.asarray(start, np.float64))


POINT_CASES = [
    _point("rejecting", "reject", 13, (0, 1, 2), (0.05, -0.03, 0.02), (-4.0, -1.0, 0.5), 1.5, 1430),  # a start far beyond the point, seen from the cameras
    _point("singular", "refused3", 9, (3, 4, 5), (0.05, -0.03, 0.02), (0.2, 0.1, 0.3), 1.0, 12),
    _point("zero_cost", "zero_cost", 17, (6, 7, 8), (1.0, 2.0, 4.0), (1.0, 2.0, 4.0), 0.0, 0),
    _point("outlier", "outlier", 5, (9, 12, 15, 18, 21, 24), (0.1, -0.2, 0.15), (0.4, 0.1, -0.2), 1.0, 13, outlier=15),
    _point("all_views", "lanes64", 4, tuple(range(32)), (0.1, -0.2, 0.3), (0.25, -0.05, 0.45), 1.0, 14),
    _point("no_cost", "nonfinite_start", 1, (6, 7, 8), (1.0, 2.0, 4.0), (1.0, 2.0, 0.0), 0.0, 0),  # h2 = z = 0 in its views: h / 0
]


# ---- the cameras ----
TRUTH = np.array([0.2, -0.1, 0.3, 0.1, -0.2, 5.0, 900.0, 880.0, 320.0, 250.0])
FAR = np.array([1.2, 0.9, -1.0, 1.0, 1.0, -2.5, -400.0, 500.0, 100.0, 100.0])
MILD = np.array([0.05, -0.04, 0.03, 0.1, -0.1, 0.3, 20.0, -15.0, 5.0, -5.0])


def _camera(name, paths, min_safe, count, start, noise, seed, truth=TRUTH, flat=False):
    rng = np.random.default_rng(seed)
    p3 = rng.uniform(-1.0, 1.0, (count, 3))
    if flat:
        p3[:, 0] = 0.0
    p2 = RC.jacobian(truth, p3)[0] + rng.normal(0.0, noise, (count, 2))
    return dict(name=name, path=paths, min_safe=min_safe, p3=p3, p2=p2, start=np.asarray(start, np.float64))


_FLAT = np.array([0.0, 0.0, 0.0, 0.0, -0.2, 5.0, 900.0, 880.0, 320.0, 250.0])  # r = 0, t_x = 0 and every X_x = 0: xn == 0 exactly, H[6][:] == 0
_NAN, _NO_FY = TRUTH.copy(), TRUTH + MILD
_NAN[5] = np.nan
_NO_FY[7] = 0.0  # v = cy whatever the pose: Jv == 0 and Ju[4] == 0, so H[4][:] == 0 exactly
# `path` and `min_safe` by n_params: the (camera, n_params) pairs that are cases.  In a mixed launch every camera runs with 6 and with 10
# parameters all the same; the pairs left out (6 parameters beside wrong intrinsics) converge linearly, with a long tail of close decisions.
CAMERA_CASES = [
    _camera("far", {10: "interleaved"}, {10: 40}, 24, TRUTH + FAR, 1.0, 109),
    _camera("stuck", {10: "step_limit"}, {10: 100}, 24, TRUTH + FAR, 1.0, 21),
    _camera("mild", {10: "iterates"}, {10: 5}, 24, TRUTH + MILD, 1.0, 22),
    _camera("mild6", {6: "iterates"}, {6: 5}, 24, TRUTH + np.r_[MILD[:6], np.zeros(4)], 1.0, 27),
    _camera("near", {6: "iterates"}, {6: 4}, 24, TRUTH + 1e-3 * MILD, 1.0, 29),  # done within the host's first poll
    _camera("flat", {10: "refused10", 6: "iterates"}, {10: 9, 6: 5}, 24, _FLAT + np.r_[np.zeros(4), 0.1, -0.3, 30.0, -20.0, 4.0, 3.0], 1.0, 23,
            truth=_FLAT, flat=True),
    _camera("fy_zero", {6: "refused6"}, {6: 9}, 24, _NO_FY, 1.0, 28),
    _camera("nan_start", {10: "nonfinite_start", 6: "nonfinite_start"}, {10: 1, 6: 1}, 24, _NAN, 1.0, 24),
    _camera("few", {10: "skipped", 6: "skipped"}, {10: 0, 6: 0}, 19, TRUTH + MILD, 1.0, 25),
    _camera("many", {10: "two_partials"}, {10: 5}, 300, TRUTH + 2.0 * MILD, 1.0, 26),
]
SMALL_CAMERAS = [c for c in CAMERA_CASES if len(c["p3"]) <= 24]  # one launch of them has n_blocks == 1
CAMERA_RUNS = [(c, n) for c in CAMERA_CASES for n in sorted(c["path"], reverse=True)]

_CACHE = {}


def point_run(case):
    """(restatement, exact-step iteration or None for a start without a finite cost) of a point case: computed once and shared."""
    key = ("point", case["name"])
    if key not in _CACHE:
        ref = RP.lm(POINT_P, case["obs"], case["mask"], case["xyz0"], F_SCALE, POINT_STEPS)
        exact = None if ref["status"] == lm_ref.NONFINITE else RP.lm_exact(POINT_P, case["obs"], case["mask"], case["xyz0"], F_SCALE, POINT_STEPS)
        _CACHE[key] = (ref, exact)
    return _CACHE[key]


def camera_run(case, n_params):
    """(restatement, exact-step iteration or None for a skipped camera or a start without a finite cost) of a camera case."""
    key = ("camera", case["name"], n_params)
    if key not in _CACHE:
        ref = RC.lm(case["start"], case["p3"], case["p2"], n_params, F_SCALE, CAMERA_STEPS)
        exact = RC.lm_exact(case["start"], case["p3"], case["p2"], n_params, F_SCALE, CAMERA_STEPS) if ref["status"] <= lm_ref.STEP_LIMIT else None
        _CACHE[key] = (ref, exact)
    return _CACHE[key]


def prefix_steps(safe):
    """The max_steps of the prefix runs: 1 .. min(safe, 20), beyond 20 only around the host's polls (every 8 pairs): 23, 24, 25, 31, ...,
    and the whole safe prefix."""
    return [k for k in range(1, safe + 1) if k <= 20 or k % 8 in (7, 0, 1) or k == safe]


def all_runs():
    """[(label, restatement, exact or None, path, min_safe)] of every case, points first."""
    out = [("point " + c["name"],) + point_run(c) + (c["path"], c["min_safe"]) for c in POINT_CASES]
    return out + [(f"camera {c['name']} p{n}",) + camera_run(c, n) + (c["path"][n], c["min_safe"][n]) for c, n in CAMERA_RUNS]
