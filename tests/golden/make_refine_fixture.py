"""Writes tests/golden/refine_cameras_ref.npz: the reference's own smal_fitter/sleap_data/refine_camera_params.py (optimize_camera,
gather_correspondences, quick_reproj_stats) on a seeded rig, in float64 as the reference runs it.  Needs scipy.

    python tests/golden/make_refine_fixture.py /path/to/reference/checkout

The two reference modules are loaded by file path.  They import h5py, toml and cv2 at their top: empty placeholder modules stand in
for the first two, and the cv2 placeholder has ONE function, a numpy restatement of ``Rodrigues`` (closed form, series below
1e-3 rad^2), because unpack_params calls it.  OpenCV itself is therefore NOT pinned by this fixture: what is pinned is scipy's
least_squares on the reference's residual function.  Every camera has dist = 0, so undistort_points returns early.

The rig: the 12 ring cameras of the triangulation fixture (same seed), the world turned so that camera 4 has R = I, i.e.
rvec = 0 exactly.  Per camera a true camera and a perturbed initial one: rotation by ~0.01 rad about a random axis (camera 4: none, its
initial rvec is exactly 0), translation ~2 cm, focal lengths +-3 %, principal point +-8 px.  Correspondences: seeded 3-D points seen
through the TRUE camera with 1 px Gaussian noise and ~8 % gross outliers (60 - 300 px).  Counts per camera hit every edge of the
accumulation kernel's 256-lane workgroups: 19 (skipped), 20, 255, 256, 257, 549 (two workgroups and 37), and six ordinary ones.

Recorded per camera, for 10 and for 6 parameters: the initial parameters, scipy's result (optimize_camera: parameters, cost, nfev,
status, the stats), and a TIGHT solution, least_squares restarted from scipy's own result with ftol = xtol = gtol = 1e-15.
Recorded for the alternation: a 40-frame x 8-keypoint scene of the same rig (1 px noise, outliers, dropouts), the reference's
gather_correspondences on it (rows and the indices its generator drew, with and without the subsample) and quick_reproj_stats.
Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_triangulate_fixture as tf  # noqa: E402  (the rig)

SEED = 31
COUNTS = (300, 19, 20, 255, 256, 257, 549, 21, 64, 100, 513, 40)
ZERO_CAM = 4
SCENE_FRAMES, SCENE_KP = 40, 8
STAT_KEYS = ("n_points", "n_evaluations", "median_err_before", "median_err_after", "pct_under_5px_before", "pct_under_5px_after",
             "pct_under_10px_before", "pct_under_10px_after")
QUICK_KEYS = ("median_px", "mean_px", "pct_under_5px", "pct_under_10px", "n_comparisons")


def rodrigues(r):
    r = np.asarray(r, np.float64).reshape(3)
    t2 = float(r @ r)
    if t2 < 1e-3:
        a = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 - t2 / 5040.0))
        b = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 - t2 / 40320.0))
    else:
        th = np.sqrt(t2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t2
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def rvec_of(R):
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    return w * (np.arctan2(s, c) / (2.0 * s)) if s > 1e-12 else np.zeros(3)


def load_reference(checkout):
    for name in ("h5py", "toml"):
        sys.modules.setdefault(name, types.ModuleType(name))
    cv2 = types.ModuleType("cv2")
    cv2.Rodrigues = lambda rvec: (rodrigues(rvec), None)
    sys.modules["cv2"] = cv2
    for pkg in ("smal_fitter", "smal_fitter.sleap_data"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    mods = {}
    for name in ("triangulate_3d_points", "refine_camera_params"):
        full = "smal_fitter.sleap_data." + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(checkout, "smal_fitter", "sleap_data", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[full] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["triangulate_3d_points"], mods["refine_camera_params"]


def project(cam, X):
    x = (cam["K"] @ (cam["R"] @ X.T + cam["t"])).T
    return x[:, :2] / x[:, 2:3]


def main():
    from scipy.optimize import least_squares

    tri, ref = load_reference(sys.argv[1])
    names = [f"cam{c:02d}" for c in range(tf.C)]
    ring = tf.rig(np.random.default_rng(tf.SEED))
    R_world = ring[names[ZERO_CAM]]["R"].copy()  # the world turned so that this camera looks along its axes
    rng = np.random.default_rng(SEED)
    true, init = {}, {}
    for c, n in enumerate(names):
        R = ring[n]["R"] @ R_world.T
        if c == ZERO_CAM:
            R = np.eye(3)
        rv = rvec_of(R)
        true[n] = dict(K=ring[n]["K"].copy(), dist=np.zeros(5), R=rodrigues(rv), t=ring[n]["t"].copy(), rvec=rv)
        axis = rng.normal(size=3)
        dR = rodrigues(0.01 * axis / np.linalg.norm(axis))
        rv0 = np.zeros(3) if c == ZERO_CAM else rvec_of(dR @ true[n]["R"])
        K0 = true[n]["K"].copy()
        K0[0, 0] *= 1.0 + rng.uniform(-0.03, 0.03)
        K0[1, 1] *= 1.0 + rng.uniform(-0.03, 0.03)
        K0[0, 2] += rng.uniform(-8.0, 8.0)
        K0[1, 2] += rng.uniform(-8.0, 8.0)
        init[n] = dict(K=K0, dist=np.zeros(5), R=rodrigues(rv0), t=true[n]["t"] + rng.normal(0.0, 0.02, (3, 1)), rvec=rv0)

    out = dict(counts=np.asarray(COUNTS), zero_cam=np.int64(ZERO_CAM), stat_keys=np.asarray(STAT_KEYS), quick_keys=np.asarray(QUICK_KEYS),
               f_scale=np.float64(5.0), true_params=np.stack([ref.pack_params(true[n]) for n in names]),
               init_params=np.stack([ref.pack_params(init[n]) for n in names]))
    pts3, pts2 = [], []
    for c, n in enumerate(names):
        X = rng.uniform(-0.5, 0.5, (COUNTS[c], 3)) @ R_world.T
        x = project(true[n], X) + rng.normal(0.0, 1.0, (COUNTS[c], 2))
        bad = rng.uniform(size=COUNTS[c]) < 0.08
        ang = rng.uniform(0.0, 2.0 * np.pi, COUNTS[c])
        x[bad] += (rng.uniform(60.0, 300.0, COUNTS[c])[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[bad]
        pts3.append(X)
        pts2.append(x)
    out["pts_3d"], out["pts_2d"] = np.concatenate(pts3), np.concatenate(pts2)
    out["offsets"] = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)

    for n_p, intr in ((10, True), (6, False)):
        res_x, tight_x, cost, tight_cost, status, stats = [], [], [], [], [], []
        for c, n in enumerate(names):
            cam, st = ref.optimize_camera(n, init[n], pts3[c], pts2[c], optimize_intrinsics=intr, verbose=False)
            x0 = ref.pack_params(init[n], intr)
            if st["status"] == "skipped":
                assert cam is init[n]
                res_x.append(x0), tight_x.append(x0), cost.append(np.nan), tight_cost.append(np.nan), status.append("skipped")
                stats.append([st["n_points"]] + [np.nan] * (len(STAT_KEYS) - 1))
                continue
            x = ref.pack_params(cam, intr)
            args = (pts3[c], pts2[c], init[n], intr)
            def loss(p):  # scipy's soft_l1 cost of a parameter vector
                z = (ref.reprojection_residuals(p, *args) / 5.0) ** 2
                return 0.5 * 25.0 * float(np.sum(2.0 * (np.sqrt(1.0 + z) - 1.0)))

            tight = least_squares(ref.reprojection_residuals, x, args=args, method="trf", loss="soft_l1", f_scale=5.0, ftol=1e-15,
                                  xtol=1e-15, gtol=1e-15, max_nfev=2000)
            res_x.append(x), tight_x.append(tight.x), cost.append(loss(x)), tight_cost.append(tight.cost), status.append(st["status"])
            stats.append([float(st[k]) for k in STAT_KEYS])
            print(n_p, n, st["status"], st["n_evaluations"], f"cost {cost[-1]:.9f} tight {tight.cost:.9f} nfev {tight.nfev}",
                  f"|x - tight| {np.abs(x - tight.x).max():.2e}")
        out[f"p{n_p}_scipy_x"], out[f"p{n_p}_tight_x"] = np.stack(res_x), np.stack(tight_x)
        out[f"p{n_p}_scipy_cost"], out[f"p{n_p}_tight_cost"] = np.asarray(cost), np.asarray(tight_cost)
        out[f"p{n_p}_status"], out[f"p{n_p}_stats"] = np.asarray(status), np.asarray(stats)

    # ---- the scene of the alternation ----
    X = rng.uniform(-0.5, 0.5, (SCENE_FRAMES, SCENE_KP, 3)) @ R_world.T
    coords = np.stack([project(true[n], X.reshape(-1, 3)).reshape(SCENE_FRAMES, SCENE_KP, 2) for n in names])
    coords += rng.normal(0.0, 1.0, coords.shape)
    scores = rng.uniform(0.5, 1.0, coords.shape[:3])
    bad = rng.uniform(size=coords.shape[:3]) < 0.08
    ang = rng.uniform(0.0, 2.0 * np.pi, coords.shape[:3])
    coords[bad] += (rng.uniform(60.0, 300.0, coords.shape[:3])[..., None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1))[bad]
    kind = rng.integers(0, 40, coords.shape[:3])
    coords[kind == 0] = np.nan
    coords[kind == 1] = 0.0
    scores[kind == 2] = 0.1
    scores[kind == 3] = np.nan
    out["scene_coords"], out["scene_scores"] = coords, scores
    all_coords = {n: coords[c] for c, n in enumerate(names)}
    all_scores = {n: scores[c] for c, n in enumerate(names)}
    tracks, _ = tri.triangulate_all(init, all_coords, all_scores, SCENE_FRAMES, SCENE_KP, confidence_threshold=0.3, min_views=3,
                                    reproj_threshold=15.0, undistort=True, use_ransac=True, verbose=False)
    out["scene_tracks"] = tracks
    kp_3d = tracks[:, 0]
    valid_3d = ~np.isnan(kp_3d).any(axis=-1) & (kp_3d != 0).any(axis=-1)

    drawn = []

    class Spy:
        def __init__(self, seed):
            self.g = np.random.default_rng(seed)

        def choice(self, *a, **kw):
            r = self.g.choice(*a, **kw)
            drawn.append(np.asarray(r))
            return r

    spy = Spy(43)
    g3, g2, gn = [], [], []
    for c, n in enumerate(names[:3]):  # the caller's generator runs on from camera to camera
        p3, p2 = ref.gather_correspondences(kp_3d, valid_3d, coords[c], scores[c], init[n], 0.3, max_points=150, rng=spy)
        g3.append(p3), g2.append(p2), gn.append(len(p3))
    out["gather_pts_3d"], out["gather_pts_2d"], out["gather_n"] = np.concatenate(g3), np.concatenate(g2), np.asarray(gn)
    out["gather_draws"] = np.stack(drawn)
    p3, p2 = ref.gather_correspondences(kp_3d, valid_3d, coords[5], scores[5], init[names[5]], 0.3)
    out["gather_full_pts_3d"], out["gather_full_pts_2d"] = p3, p2
    q = ref.quick_reproj_stats(tracks, all_coords, all_scores, init, 0.3, max_points_per_cam=200)
    out["quick_stats"] = np.asarray([float(q[k]) for k in QUICK_KEYS])

    path = os.path.join(HERE, "refine_cameras_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
