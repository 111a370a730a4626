"""Multi-view keypoint triangulation on the HIP kernel: the array-level functions of the reference's
``smal_fitter/sleap_data/triangulate_3d_points.py`` ("Core triangulation loop (reusable from other scripts)", :826-978), name for name.

``triangulate_all`` runs every (frame, keypoint) problem of a session in one launch of ``csrc/triangulate.hip``; the single-point
functions run the same kernel on one problem.  Everything is float64, and there is no CPU path: the arrays go to ``device`` (default
``cuda:0``) and the results come back as numpy.  File readers (calibration ``.toml``, SLEAP ``.h5`` / ``.slp``) are out of scope.
Deviations from the reference:

* at most ``SMIL_TRI_MAX_VIEWS`` cameras, and ``max_hypotheses`` is the reference's default of 50;
* the undistortion is the documented five-round recurrence of ``cv2.undistortPoints``, not a call into OpenCV;
* among hypotheses of equal inlier count the lowest index wins (what the reference's strict ``>`` keeps, stated as a rule);
* non-finite projection matrices or infinite observations give NaN points where ``numpy.linalg.svd`` raises;
* ``reprojection_errors_vectorized`` / ``reprojection_error`` of a GIVEN point are three numpy lines on the host;
* a calibration with non-zero distortion coefficients beyond the first five raises ``NotImplementedError``.
"""
from __future__ import annotations

import itertools
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, engine

__all__ = ["get_projection_matrix", "triangulate_point_dlt", "reprojection_errors_vectorized", "reprojection_error",
           "triangulate_point_ransac", "undistort_points", "triangulate_all", "projection_matrix_from_fov_camera", "pair_table",
           "triangulate_arrays"]

DEFAULT_DEVICE = "cuda:0"
_PAIR_TABLE: Optional[np.ndarray] = None
_PAIR_TABLE_DEV: Dict = {}


def pair_table() -> np.ndarray:
    """(SMIL_TRI_MAX_VIEWS + 1, SMIL_TRI_MAX_HYP, 2) int32: row n holds the hypotheses of n valid views (:240-245), all pairs of
    ``itertools.combinations(range(n), 2)`` or, above 50 of them, ``np.random.default_rng(42).choice(len, 50, replace=False)`` of that
    list.  Rows 0, 1 and the entries behind a row's last pair are zero."""
    global _PAIR_TABLE
    if _PAIR_TABLE is None:
        table = np.zeros((_lib.TRI_MAX_VIEWS + 1, _lib.TRI_MAX_HYP, 2), np.int32)
        for n in range(2, _lib.TRI_MAX_VIEWS + 1):
            pairs = list(itertools.combinations(range(n), 2))
            if len(pairs) > _lib.TRI_MAX_HYP:
                rng = np.random.default_rng(42)
                pairs = [pairs[i] for i in rng.choice(len(pairs), _lib.TRI_MAX_HYP, replace=False)]
            table[n, :len(pairs)] = pairs
        table.setflags(write=False)
        _PAIR_TABLE = table
    return _PAIR_TABLE


def _pair_table_on(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index)
    if key not in _PAIR_TABLE_DEV:
        _PAIR_TABLE_DEV[key] = torch.from_numpy(pair_table().copy()).to(device)
    return _PAIR_TABLE_DEV[key]


def get_projection_matrix(cam: dict) -> np.ndarray:
    """The 3 x 4 projection ``K @ [R | t]`` of a calibration entry (:68-71).  An entry that carries a ready matrix under ``"P"`` (an
    extension: ``projection_matrix_from_fov_camera``) hands that back."""
    if "P" in cam:
        return np.asarray(cam["P"], np.float64).reshape(3, 4)
    return np.asarray(cam["K"], np.float64) @ np.hstack([np.asarray(cam["R"], np.float64), np.asarray(cam["t"], np.float64).reshape(3, 1)])


def projection_matrix_from_fov_camera(R, T, fov, aspect_ratio=1.0, image_size=512, principal_point=None) -> np.ndarray:
    """The 3 x 4 pixel projection of one FoV camera of this library: ``X_view = X R + T`` (row vectors),
    ``x_ndc = X_view.x / (aspect tan(fov / 2) X_view.z)``, ``y_ndc = X_view.y / (tan(fov / 2) X_view.z)`` and the screen transform
    ``x = W/2 - (W/2) x_ndc``, ``y = H/2 - (H/2) y_ndc`` of ``Renderer.forward(..., joints_only=True)``, whose output is ``(y, x)``.
    ``P @ [X, 1]`` is ``(x w, y w, w)``: tracks triangulated through it live in the frame the fitter renders in.  fov in degrees;
    image_size an int or ``(H, W)``.  ``principal_point = (px, py)``: the camera's NDC offset (``x_ndc + px``, ``y_ndc + py``; None:
    centred), so that a camera handed to the renderer with it and to ``triangulate_all`` describes the same pixels."""
    R = np.asarray(torch.as_tensor(R).detach().cpu().numpy(), np.float64).reshape(3, 3)
    T = np.asarray(torch.as_tensor(T).detach().cpu().numpy(), np.float64).reshape(3)
    H, W = (image_size, image_size) if np.isscalar(image_size) else image_size
    t = np.tan(np.radians(float(fov)) / 2.0)
    k00, k11 = 1.0 / (float(aspect_ratio) * t), 1.0 / t
    rows = np.hstack([R.T, T[:, None]])  # row i: X_view[i] = rows[i] . [X, 1]
    if principal_point is None:
        return np.stack([0.5 * W * (rows[2] - k00 * rows[0]), 0.5 * H * (rows[2] - k11 * rows[1]), rows[2]])
    px, py = (float(v) for v in np.asarray(torch.as_tensor(principal_point).detach().cpu().numpy(), np.float64).reshape(2))
    return np.stack([0.5 * W * ((1.0 - px) * rows[2] - k00 * rows[0]), 0.5 * H * ((1.0 - py) * rows[2] - k11 * rows[1]), rows[2]])


def triangulate_arrays(P, obs, scores=None, K=None, dist=None, confidence_threshold=0.3, min_views=2, reproj_threshold=15.0,
                       use_ransac=True, keep_all_views=False, device=None, refine=False) -> Dict[str, np.ndarray]:
    """The kernel on numpy arrays: P (C,3,4), obs (N,Kp,C,2), scores (N,Kp,C) or None, K (C,3,3) and dist (C,5) or None.  Returns
    ``xyz, status, views_used, mean_err, view_err, inlier_mask`` (uint32, bit c = camera c is in the final system) and
    ``obs_undistorted`` (the valid views' points as they entered the systems, NaN for a dropped view) as numpy.

    ``refine=True`` (an extension, ``smilify_amd/refine_points.py``): every triangulated point is then moved from the DLT point to the
    minimum of the soft_l1 reprojection cost over the views of its final system (``inlier_mask``).  ``status``, ``views_used`` and
    ``inlier_mask`` stay, ``view_err`` and ``mean_err`` are those of the refined point over the same valid views as before, and the
    dict gains ``refine_status``, ``refine_cost_initial`` and ``refine_cost_final`` (N,Kp)."""
    dev = engine.require_gpu(device or DEFAULT_DEVICE)
    up = lambda x: engine.upload_f64(x, dev)  # noqa: E731
    mode = (_lib.TRI_RANSAC if use_ransac else 0) | (_lib.TRI_KEEP_ALL_VIEWS if keep_all_views else 0)
    obs = np.asarray(obs, np.float64)
    if obs.ndim != 4 or obs.shape[3] != 2:
        raise ValueError("triangulate_arrays: obs must be (N, Kp, C, 2)")
    if obs.shape[2] > _lib.TRI_MAX_VIEWS:
        raise ValueError(f"triangulate: {obs.shape[2]} cameras above SMIL_TRI_MAX_VIEWS={_lib.TRI_MAX_VIEWS}")
    out = engine.triangulate(up(P), up(obs), up(scores), _pair_table_on(dev) if use_ransac else None, K=up(K), dist=up(dist),
                             confidence_threshold=confidence_threshold, min_views=min_views, reproj_threshold=reproj_threshold,
                             mode=mode, want_view_err=True, want_inlier_mask=True, want_undistorted=True)
    xyz, status, used, mean_err, view_err, mask, undist = (t.cpu().numpy() for t in out)
    out = dict(xyz=xyz, status=status, views_used=used, mean_err=mean_err, view_err=view_err, inlier_mask=mask.view(np.uint32),
               obs_undistorted=undist)
    if refine:
        _refine_in_place(np.asarray(P, np.float64).reshape(-1, 3, 4), out, dev)
    return out


def _refine_in_place(P: np.ndarray, out: Dict[str, np.ndarray], device) -> None:
    """The refined points in place of the DLT points of ``out`` where the refinement ran (status 0 or 1), with their errors."""
    from . import refine_points as rp

    xyz, st = rp.refine_points_arrays(P, out["obs_undistorted"], out["inlier_mask"], out["xyz"], device=device)
    moved = (out["status"] == 0) & ((st["status"] == _lib.REFINE_CONVERGED) | (st["status"] == _lib.REFINE_STEP_LIMIT))
    out.update(refine_status=st["status"], refine_cost_initial=st["cost_initial"], refine_cost_final=st["cost_final"])
    if not moved.any():
        return
    X, und = xyz[moved], out["obs_undistorted"][moved]
    valid = ~np.isnan(und).any(axis=-1)  # the views that entered the hypotheses: mean_err runs over all of them
    with np.errstate(all="ignore"):
        h = np.einsum("cij,mj->mci", P[:, :, :3], X) + P[:, :, 3]
        err = np.where(valid, np.linalg.norm(h[..., :2] / h[..., 2:3] - und, axis=-1), np.nan)
    out["xyz"][moved], out["view_err"][moved] = X, err
    out["mean_err"][moved] = np.where(valid, err, 0.0).sum(axis=-1) / valid.sum(axis=-1)


def _one_problem(projections, points_2d):
    P = np.asarray(projections, np.float64).reshape(-1, 3, 4)
    pts = np.asarray(points_2d, np.float64).reshape(-1, 2)
    if len(P) != len(pts):
        raise ValueError("one projection matrix per 2-D point")
    return P, pts[None, None]


def triangulate_point_dlt(projections, points_2d) -> np.ndarray:
    """DLT triangulation of one point from N >= 2 views (:156-176): projections N x (3, 4), points_2d N x (2,); (3,) float64."""
    P, obs = _one_problem(projections, points_2d)
    return triangulate_arrays(P, obs, min_views=1, use_ransac=False, keep_all_views=True)["xyz"][0, 0]


def reprojection_errors_vectorized(Ps, pt_3d, pts_2d) -> np.ndarray:
    """(N,) reprojection errors in pixels of the GIVEN point pt_3d (3,) in the views Ps (N, 3, 4) against pts_2d (N, 2) (:179-194)."""
    proj = np.asarray(Ps, np.float64) @ np.append(np.asarray(pt_3d, np.float64), 1.0)
    return np.linalg.norm(proj[:, :2] / proj[:, 2:3] - np.asarray(pts_2d, np.float64), axis=1)


def reprojection_error(P, pt_3d, pt_2d) -> float:
    """The reprojection error of one view (:197-202)."""
    return float(reprojection_errors_vectorized(np.asarray(P)[None], pt_3d, np.asarray(pt_2d)[None])[0])


def triangulate_point_ransac(Ps_arr, pts_arr, reproj_threshold: float = 15.0, min_inliers: int = 2,
                             max_hypotheses: int = 50) -> Tuple[Optional[np.ndarray], int]:
    """Pair-RANSAC triangulation of one point (:205-281): ``(pt_3d, n_inliers)`` or ``(None, 0)``."""
    if max_hypotheses != _lib.TRI_MAX_HYP:
        raise NotImplementedError(f"max_hypotheses is fixed at SMIL_TRI_MAX_HYP={_lib.TRI_MAX_HYP}")
    n = len(Ps_arr)
    if n < 2:
        return None, 0
    P, obs = _one_problem(Ps_arr, pts_arr)
    if n == 2:  # the reference's own branch: the pair's point, accepted by its count of inliers
        out = triangulate_arrays(P, obs, min_views=1, use_ransac=False, keep_all_views=True)
        n_inliers = int((out["view_err"][0, 0] < reproj_threshold).sum())
        return (out["xyz"][0, 0], n_inliers) if n_inliers >= min_inliers else (None, 0)
    out = triangulate_arrays(P, obs, min_views=max(1, int(min_inliers)), reproj_threshold=reproj_threshold, use_ransac=True,
                             keep_all_views=True)
    if int(out["status"][0, 0]) != 0:
        return None, 0
    return out["xyz"][0, 0], int(out["views_used"][0, 0])


def undistort_points(points_2d, K, dist) -> np.ndarray:
    """(N, 2) pixel coordinates undistorted by the calibration (:284-301); unchanged when dist is None or all close to zero.

    The recurrence lives in the kernel's load phase and nowhere else, so the points go through it as N one-camera problems with
    ``min_views=1``: each wave also solves a rank-2 system whose point is thrown away, and only ``obs_undistorted`` is read back.
    That output of ``smil_triangulate`` exists for this function and for the test that pins the recurrence; ``triangulate_all``
    does not go through here, it undistorts inside its own launch."""
    points_2d = np.asarray(points_2d)
    if dist is None or np.allclose(dist, 0):
        return points_2d
    pts = points_2d.reshape(-1, 1, 1, 2).astype(np.float64)
    out = triangulate_arrays(np.eye(3, 4)[None], pts, K=np.asarray(K, np.float64).reshape(1, 3, 3), dist=_dist5(dist)[None], min_views=1,
                             use_ransac=False, keep_all_views=True)
    return out["obs_undistorted"].reshape(-1, 2)


def _dist5(dist) -> np.ndarray:
    d = np.zeros(5, np.float64)
    if dist is not None:
        flat = np.ravel(np.asarray(dist, np.float64))
        if flat.size > 5 and np.any(flat[5:] != 0):
            raise NotImplementedError("undistortion takes the five coefficients (k1, k2, p1, p2, k3)")
        d[:min(5, flat.size)] = flat[:5]
    return d


def triangulate_all(cameras: Dict[str, dict], all_coords: Dict[str, np.ndarray], all_scores: Dict[str, np.ndarray], n_frames: int,
                    n_keypoints: int, confidence_threshold: float = 0.3, min_views: int = 2, reproj_threshold: float = 15.0,
                    undistort: bool = True, use_ransac: bool = True, verbose: bool = True,
                    frame_indices: Optional[np.ndarray] = None, device=None, refine: bool = False) -> Tuple[np.ndarray, dict]:
    """Triangulate every keypoint of every frame (:830-978): ``cameras`` name -> {K, dist, R, t}, ``all_coords`` name ->
    (n_frames_cam, n_kp, 2), ``all_scores`` name -> (n_frames_cam, n_kp).  Returns ``tracks_3d (n_out, 1, n_keypoints, 3)`` float64,
    NaN where not triangulated, and the reference's ``stats`` dict.  Cameras are taken in ``sorted(all_coords)`` order; a frame
    beyond a camera's own frame count is a dropped view.  ``refine=True`` (an extension): the points are refined as
    ``triangulate_arrays(refine=True)`` describes, the error statistics are those of the refined points, and the stats gain
    ``refined``, the number of points that moved."""
    start = time.time()
    names = sorted(all_coords.keys())
    C = len(names)
    if C > _lib.TRI_MAX_VIEWS:
        raise ValueError(f"triangulate_all: {C} cameras above SMIL_TRI_MAX_VIEWS={_lib.TRI_MAX_VIEWS}")
    frame_indices = np.arange(n_frames) if frame_indices is None else np.asarray(frame_indices)
    n_out = len(frame_indices)
    stats = {"n_frames": n_out, "n_keypoints": n_keypoints, "n_cameras": C, "total_keypoints": n_out * n_keypoints, "triangulated": 0,
             "failed_insufficient_views": 0, "failed_ransac": 0}
    tracks_3d = np.full((n_out, 1, n_keypoints, 3), np.nan, dtype=np.float64)
    if verbose:
        print(f"\n  Triangulating {n_out} frames x {n_keypoints} keypoints using {C} cameras")
        print(f"  Confidence threshold: {confidence_threshold}\n  Min views: {min_views}\n  Reproj threshold: {reproj_threshold} px")
        print(f"  Undistort 2D before triangulation: {undistort}\n  Method: {'RANSAC' if use_ransac else 'DLT'}")
    vu = re = np.zeros(0)
    if n_out > 0 and n_keypoints > 0 and C > 0:
        obs = np.full((n_out, n_keypoints, C, 2), np.nan, np.float64)
        scores = np.full((n_out, n_keypoints, C), np.nan, np.float64)
        for c, name in enumerate(names):
            coords, sc = np.asarray(all_coords[name]), np.asarray(all_scores[name])
            have = frame_indices < coords.shape[0]  # :909-910
            obs[have, :, c] = coords[frame_indices[have], :n_keypoints]
            scores[have, :, c] = sc[frame_indices[have], :n_keypoints]
        P = np.stack([get_projection_matrix(cameras[name]) for name in names])
        K = dist = None
        if undistort:
            K = np.stack([np.asarray(cameras[name].get("K", np.eye(3)), np.float64).reshape(3, 3) for name in names])
            dist = np.stack([_dist5(cameras[name].get("dist")) for name in names])
        out = triangulate_arrays(P, obs, scores, K, dist, confidence_threshold, min_views, reproj_threshold, use_ransac, device=device,
                                 refine=refine)
        ok = out["status"] == 0
        if refine:
            stats["refined"] = int((ok & (out["refine_status"] <= _lib.REFINE_STEP_LIMIT)).sum())
        tracks_3d[:, 0][ok] = out["xyz"][ok]
        stats["failed_insufficient_views"] = int((out["status"] == 1).sum())
        stats["failed_ransac"] = int((out["status"] == 2).sum())
        vu, re = out["views_used"][ok], out["mean_err"][ok]  # frame-major, the order the reference appends in
    stats["triangulated"] = int(len(vu))
    stats["pct_triangulated"] = 100.0 * stats["triangulated"] / max(1, stats["total_keypoints"])
    stats["mean_views_used"] = float(np.mean(vu)) if len(vu) else 0
    stats["mean_reproj_error_px"] = float(np.mean(re)) if len(re) else 0
    stats["median_reproj_error_px"] = float(np.median(re)) if len(re) else 0
    if verbose:
        print(f"\n  Triangulation completed in {time.time() - start:.1f}s")
        print(f"  Triangulated: {stats['triangulated']} / {stats['total_keypoints']} ({stats['pct_triangulated']:.1f}%)")
        print(f"  Failed (insufficient views): {stats['failed_insufficient_views']}")
        print(f"  Failed (RANSAC):             {stats['failed_ransac']}")
        print(f"  Mean views used:  {stats['mean_views_used']:.1f}")
        print(f"  Mean reproj err:  {stats['mean_reproj_error_px']:.2f} px")
        print(f"  Median reproj err: {stats['median_reproj_error_px']:.2f} px")
    return tracks_3d, stats
