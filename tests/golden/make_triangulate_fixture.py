"""Writes tests/golden/triangulate_ref.npz: the reference's own smal_fitter/sleap_data/triangulate_3d_points.py on a seeded rig, in
float64 as the reference runs it.

    python tests/golden/make_triangulate_fixture.py /path/to/reference/checkout

The module imports h5py, cv2 and toml at its top for its file readers; empty placeholder modules stand in for them.  Every fixture
camera has dist = 0, so undistort_points returns early and cv2 is never called.

The rig: 12 look-at cameras on a ring (66 pairs > 50: the seeded subset of hypotheses), run a second time with the first 5 cameras
only (10 pairs, all used).  6 frames x 8 keypoints of seeded 3-D points, Gaussian pixel noise of 1 px, per problem 0 - 3 views
replaced by gross outliers (> 100 px away), seeded dropouts by NaN, by a low score and by an exact (0, 0), camera 3 with 4 frames
only, and problems engineered to each failure: one valid view (frame 0, keypoint 0) and three valid views that all disagree (frame 0,
keypoint 1).  Recorded: the inputs; triangulate_all's tracks and stats for {RANSAC, plain DLT} x {min_views 2, 3} on both rigs; the
reference's draw of 50 of the 66 pairs; and for 10 single problems triangulate_point_ransac's point and inlier count.  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20
C, FRAMES, KP, SHORT_CAM, SHORT_FRAMES = 12, 6, 8, 3, 4
W, H, F = 1280.0, 1024.0, 1100.0
STAT_KEYS = ("n_frames", "n_keypoints", "n_cameras", "total_keypoints", "triangulated", "failed_insufficient_views", "failed_ransac",
             "pct_triangulated", "mean_views_used", "mean_reproj_error_px", "median_reproj_error_px")


def load_reference(checkout):
    for name in ("h5py", "cv2", "toml"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location(
        "triangulate_3d_points", os.path.join(checkout, "smal_fitter", "sleap_data", "triangulate_3d_points.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def look_at(eye):
    """OpenCV extrinsics (x_cam = R x + t, z forward, y down) of a camera at `eye` looking at the origin."""
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, (-R @ eye).reshape(3, 1)


def rig(rng):
    cams = {}
    for c in range(C):
        az = 2.0 * np.pi * c / C + rng.uniform(-0.05, 0.05)
        eye = np.array([4.0 * np.cos(az), 4.0 * np.sin(az), 1.5 + 0.5 * (c % 3)])
        R, t = look_at(eye)
        f = F * rng.uniform(0.9, 1.1)
        K = np.array([[f, 0.0, W / 2], [0.0, f * rng.uniform(0.98, 1.02), H / 2], [0.0, 0.0, 1.0]])
        cams[f"cam{c:02d}"] = dict(K=K, dist=np.zeros(5), R=R, t=t)
    return cams


def project(cam, X):
    x = cam["K"] @ (cam["R"] @ X + cam["t"][:, 0])
    return x[:2] / x[2]


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    cams = rig(rng)
    names = sorted(cams)
    X = rng.uniform(-0.5, 0.5, (FRAMES, KP, 3))
    coords = np.zeros((C, FRAMES, KP, 2))
    scores = rng.uniform(0.5, 1.0, (C, FRAMES, KP))
    for c, name in enumerate(names):
        for f in range(FRAMES):
            for k in range(KP):
                coords[c, f, k] = project(cams[name], X[f, k]) + rng.normal(0.0, 1.0, 2)
    for f in range(FRAMES):
        for k in range(KP):
            for c in rng.permutation(C)[:rng.integers(0, 4)]:  # gross outliers
                ang = rng.uniform(0.0, 2.0 * np.pi)
                coords[c, f, k] += rng.uniform(120.0, 400.0) * np.array([np.cos(ang), np.sin(ang)])
            drops = rng.permutation(C)[:rng.integers(0, 4)]
            for c in drops:
                kind = rng.integers(0, 4)
                if kind == 0:
                    coords[c, f, k, rng.integers(0, 2)] = np.nan
                elif kind == 1:
                    scores[c, f, k] = rng.uniform(0.0, 0.25)
                elif kind == 2:
                    coords[c, f, k] = 0.0
                else:
                    scores[c, f, k] = np.nan  # an unknown score keeps the view (:917)
    # one valid view: every camera but one dropped, by each of the three ways in turn
    for c in range(1, C):
        if c % 3 == 0:
            coords[c, 0, 0] = np.nan
        elif c % 3 == 1:
            scores[c, 0, 0] = 0.1
        else:
            coords[c, 0, 0] = 0.0
    coords[0, 0, 0], scores[0, 0, 0] = project(cams[names[0]], X[0, 0]), 0.9
    # three valid views that all disagree: each sees a different 3-D point
    for c in range(C):
        if c in (1, 5, 9):
            coords[c, 0, 1], scores[c, 0, 1] = project(cams[names[c]], X[0, 1] + rng.uniform(-0.6, 0.6, 3)), 0.9
        else:
            coords[c, 0, 1] = np.nan
    # the same two failures inside the first five cameras (frame 1, keypoints 0 and 1)
    for c in range(C):
        if c == 2:
            coords[c, 1, 0], scores[c, 1, 0] = project(cams[names[c]], X[1, 0]), 0.9
        elif c in (0, 1, 4):
            coords[c, 1, 1], scores[c, 1, 1] = project(cams[names[c]], X[1, 1] + rng.uniform(-0.6, 0.6, 3)), 0.9
        if c != 2:
            coords[c, 1, 0] = np.nan
        if c not in (0, 1, 4):
            scores[c, 1, 1] = 0.05

    frames_of = [SHORT_FRAMES if c == SHORT_CAM else FRAMES for c in range(C)]
    all_coords = {n: coords[c, :frames_of[c]].copy() for c, n in enumerate(names)}
    all_scores = {n: scores[c, :frames_of[c]].copy() for c, n in enumerate(names)}
    out = dict(K=np.stack([cams[n]["K"] for n in names]), R=np.stack([cams[n]["R"] for n in names]),
               t=np.stack([cams[n]["t"] for n in names]), coords=coords, scores=scores, frames_of=np.asarray(frames_of), X_true=X,
               confidence_threshold=np.float64(0.3), reproj_threshold=np.float64(15.0), stat_keys=np.asarray(STAT_KEYS))

    for ncam in (C, 5):
        sub = names[:ncam]
        for use_ransac in (True, False):
            for min_views in (2, 3):
                tracks, stats = ref.triangulate_all({n: cams[n] for n in sub}, {n: all_coords[n] for n in sub}, {n: all_scores[n] for n in sub},
                                                    FRAMES, KP, confidence_threshold=0.3, min_views=min_views, reproj_threshold=15.0,
                                                    undistort=True, use_ransac=use_ransac, verbose=False)
                key = f"all_c{ncam}_{'ransac' if use_ransac else 'dlt'}_mv{min_views}"
                out[key + "_tracks"] = tracks
                out[key + "_stats"] = np.asarray([float(stats[k]) for k in STAT_KEYS])

    # the reference's draw of the hypotheses for n = 12, seen through its own call of the generator
    drawn = []
    real_rng = np.random.default_rng

    class Spy:
        def __init__(self, seed):
            self.g = real_rng(seed)

        def choice(self, *a, **kw):
            r = self.g.choice(*a, **kw)
            drawn.append(np.asarray(r))
            return r

    Ps = np.stack([ref.get_projection_matrix(cams[n]) for n in names])
    out["P"] = Ps
    np.random.default_rng = Spy
    try:
        ref.triangulate_point_ransac(Ps, np.stack([project(cams[n], X[2, 2]) for n in names]))
    finally:
        np.random.default_rng = real_rng
    out["draw_n12"] = drawn[0].astype(np.int32)

    # ten single problems through triangulate_point_ransac: n = 2 (its own branch), small n, n = 12, one that fails
    single_views, single_pt, single_n, single_min = [], [], [], []
    picks = [(2, 3, 3, 2), (2, 3, 4, 2), (3, 3, 5, 2), (4, 2, 6, 2), (10, 4, 1, 2), (11, 4, 2, 2), (12, 5, 3, 2), (12, 5, 4, 3),
             ((1, 5, 9), 0, 1, 3), (3, 4, 6, 2)]
    for views, f, k, mn in picks:
        if isinstance(views, int):  # the first cameras whose coordinates are finite here
            views = tuple(np.flatnonzero(np.isfinite(coords[:, f, k]).all(axis=1))[:views])
        v = np.asarray(views)
        pts = coords[v, f, k]
        assert np.isfinite(pts).all(), (views, f, k)
        pt, n_in = ref.triangulate_point_ransac(Ps[v], pts, reproj_threshold=15.0, min_inliers=mn)
        mask = np.zeros(C, bool)
        mask[v] = True
        single_views.append(mask)
        single_pt.append(np.full(3, np.nan) if pt is None else pt)
        single_n.append(n_in)
        single_min.append(mn)
    out["single_views"], out["single_frame_kp"] = np.asarray(single_views), np.asarray([(f, k) for _, f, k, _ in picks])
    out["single_pt"], out["single_n"], out["single_min"] = np.asarray(single_pt), np.asarray(single_n), np.asarray(single_min)

    path = os.path.join(HERE, "triangulate_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
