"""Multi-view camera refinement on the HIP kernels: the array-level functions of the reference's
``smal_fitter/sleap_data/refine_camera_params.py``, name for name, and the loop of its ``main()`` without file I/O.

``optimize_cameras`` fits every camera of a rig in one call of ``csrc/refine.hip``; ``optimize_camera`` is the same call with one
camera.  Everything is float64, numpy in and numpy out, and there is no CPU path for the fit itself (the mask logic of
``gather_correspondences`` and the packing stay in numpy, as in the reference).  Deviations from the reference (DESIGN.md
section 4.7):

* the optimiser is a Levenberg-Marquardt on the same soft-L1 cost, not scipy's trust-region-reflective: it ends at the same minimum
  (at or below scipy's cost), not at scipy's iterates;
* the Jacobian is analytic, not 11 residual evaluations;
* ``cv2.Rodrigues`` is replaced by a numpy Rodrigues with a series for small angles (OpenCV is not a dependency);
* ``n_evaluations`` is the number of evaluations of the cost (trial steps, the first one at the initial parameters included);
* ``status`` is ``"success"`` when the iteration converged and ``"converged"`` when it ran into ``max_steps`` (the reference's two
  words for scipy's ``result.success`` and its negation), ``"skipped"`` below 20 points as in the reference, and ``"non_finite"``
  when the initial cost is not finite (scipy raises there).
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, engine
from . import triangulate as tri

__all__ = ["gather_correspondences", "pack_params", "unpack_params", "reprojection_residuals", "optimize_camera", "optimize_cameras",
           "quick_reproj_stats", "refine_cameras", "rodrigues", "rotation_to_rvec", "evaluate_cost"]

_SMALL_ANGLE2 = 1e-3


def rodrigues(rvec) -> np.ndarray:
    """The rotation matrix of an axis-angle vector: ``I + a K + b K^2`` with ``K = [rvec]x``, ``a = sin(th) / th`` and
    ``b = (1 - cos(th)) / th^2``; below ``th^2 = 1e-3`` a and b come from their series, so ``rvec = 0`` gives exactly I."""
    r = np.asarray(rvec, np.float64).reshape(3)
    t2 = float(r @ r)
    if t2 < _SMALL_ANGLE2:
        a = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 - t2 / 5040.0))
        b = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 - t2 / 40320.0))
    else:
        th = np.sqrt(t2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t2
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def rotation_to_rvec(R) -> np.ndarray:
    """The axis-angle vector (angle in [0, pi]) of a rotation matrix, for calibrations that carry ``R`` and no ``rvec``."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if s > 1e-6:
        return w * (th / (2.0 * s))
    if c > 0.0:
        return 0.5 * w  # th / sin(th) -> 1
    axis = np.sqrt(np.maximum((np.diag(R) + 1.0) / 2.0, 0.0))  # th = pi: R = 2 n n^T - I
    k = int(np.argmax(axis))
    axis = np.where((R[k] + R[:, k]) < 0.0, -axis, axis)
    axis[k] = abs(axis[k])
    return th * axis / np.linalg.norm(axis)


def gather_correspondences(kp_3d: np.ndarray, valid_3d: np.ndarray, coords_2d: np.ndarray, scores_2d: np.ndarray, cam: dict,
                           confidence_threshold: float = 0.3, max_points: Optional[int] = None,
                           rng: Optional[np.random.Generator] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Matched 3-D / 2-D correspondences of one camera (:48-96): ``pts_3d (M, 3)`` and the undistorted ``pts_2d (M, 2)``."""
    n_compare = min(kp_3d.shape[0], coords_2d.shape[0])
    sub_2d, sub_sc = coords_2d[:n_compare], scores_2d[:n_compare]
    with np.errstate(invalid="ignore"):
        both = valid_3d[:n_compare] & ~np.isnan(sub_2d).any(axis=-1) & (sub_2d != 0).any(axis=-1) \
            & (np.isnan(sub_sc) | (sub_sc >= confidence_threshold))
    fi, ki = np.where(both)
    if len(fi) == 0:
        return np.zeros((0, 3)), np.zeros((0, 2))
    pts_3d, pts_2d = kp_3d[fi, ki], tri.undistort_points(coords_2d[fi, ki], cam["K"], cam["dist"])
    if max_points is not None and len(pts_3d) > max_points:
        if rng is None:
            rng = np.random.default_rng(42)
        idx = rng.choice(len(pts_3d), max_points, replace=False)
        pts_3d, pts_2d = pts_3d[idx], pts_2d[idx]
    return pts_3d, pts_2d


def _rvec_of(cam: dict) -> np.ndarray:
    return np.asarray(cam["rvec"], np.float64).ravel() if "rvec" in cam else rotation_to_rvec(cam["R"])


def pack_params(cam: dict, optimize_intrinsics: bool = True) -> np.ndarray:
    """The flat parameter vector of a camera (:104-114): rvec, t and, with the intrinsics, fx, fy, cx, cy.  A camera without
    ``"rvec"`` (an extension) gets the axis-angle of its ``"R"``."""
    ext = np.concatenate([_rvec_of(cam), np.asarray(cam["t"], np.float64).ravel()])
    if not optimize_intrinsics:
        return ext
    K = np.asarray(cam["K"], np.float64)
    return np.concatenate([ext, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]])


def unpack_params(params: np.ndarray, cam_template: dict, optimize_intrinsics: bool = True) -> dict:
    """A copy of cam_template with the flat vector written back (:117-135)."""
    cam = copy.deepcopy(cam_template)
    params = np.asarray(params, np.float64)
    cam["rvec"] = params[:3]
    cam["t"] = params[3:6].reshape(3, 1)
    cam["R"] = rodrigues(cam["rvec"])
    if optimize_intrinsics:
        fx, fy, cx, cy = params[6:10]
        cam["K"] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
    return cam


def reprojection_residuals(params: np.ndarray, pts_3d: np.ndarray, pts_2d: np.ndarray, cam_template: dict,
                           optimize_intrinsics: bool = True) -> np.ndarray:
    """(2 M,) projected - observed, x and y interleaved (:143-163)."""
    cam = unpack_params(params, cam_template, optimize_intrinsics)
    P = tri.get_projection_matrix({"K": cam["K"], "R": cam["R"], "t": cam["t"]})
    with np.errstate(all="ignore"):
        proj = (P @ np.hstack([pts_3d, np.ones((pts_3d.shape[0], 1))]).T).T
        return (proj[:, :2] / proj[:, 2:3] - pts_2d).ravel()


def _params10(cam: dict) -> np.ndarray:
    return pack_params(cam, True)


def _pack_batch(correspondences: Sequence[Tuple[np.ndarray, np.ndarray]]):
    counts = [len(p3) for p3, _ in correspondences]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    p3 = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p, _ in correspondences]) if offsets[-1] else np.zeros((0, 3))
    p2 = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for _, p in correspondences]) if offsets[-1] else np.zeros((0, 2))
    return p3, p2, offsets


def evaluate_cost(params, correspondences, optimize_intrinsics: bool = True, f_scale: float = 5.0, device=None):
    """One accumulation of the kernel at params (C, 10): ``cost (C), g (C, 10), H (C, 10, 10)`` as numpy (entries outside the fitted
    block are zero)."""
    dev = engine.require_gpu(device or tri.DEFAULT_DEVICE)
    p3, p2, offsets = _pack_batch(correspondences)
    up = lambda x: engine.upload_f64(x, dev)  # noqa: E731
    out = engine.refine_evaluate(up(p3), up(p2), offsets, up(np.asarray(params, np.float64).reshape(-1, 10)),
                                 n_params=10 if optimize_intrinsics else 6, f_scale=f_scale)
    return tuple(t.cpu().numpy() for t in out)


def _error_stats(res0: np.ndarray, res1: np.ndarray) -> dict:
    err0, err1 = np.sqrt(res0[::2] ** 2 + res0[1::2] ** 2), np.sqrt(res1[::2] ** 2 + res1[1::2] ** 2)
    return {"median_err_before": float(np.median(err0)), "median_err_after": float(np.median(err1)),
            "pct_under_5px_before": float(100 * (err0 < 5).mean()), "pct_under_5px_after": float(100 * (err1 < 5).mean()),
            "pct_under_10px_before": float(100 * (err0 < 10).mean()), "pct_under_10px_after": float(100 * (err1 < 10).mean())}


_STATUS = {_lib.REFINE_CONVERGED: "success", _lib.REFINE_STEP_LIMIT: "converged", _lib.REFINE_SKIPPED: "skipped",
           _lib.REFINE_NONFINITE: "non_finite"}


def optimize_cameras(cameras: Dict[str, dict], correspondences: Dict[str, Tuple[np.ndarray, np.ndarray]],
                     optimize_intrinsics: bool = True, verbose: bool = True, f_scale: float = 5.0, max_steps: int = 100,
                     device=None) -> Tuple[Dict[str, dict], Dict[str, dict]]:
    """Every camera of ``correspondences`` (name -> (pts_3d, pts_2d)) in one launch: ``(refined cameras, stats)`` by name, each
    as ``optimize_camera`` returns them.  A skipped or non-finite camera is returned as it came.  The stats carry, beyond the
    reference's keys, ``cost_initial``, ``cost_final``, ``n_accepted`` and ``gradient`` (the final g)."""
    names = [n for n in sorted(cameras) if n in correspondences]
    if not names:
        return {}, {}
    dev = engine.require_gpu(device or tri.DEFAULT_DEVICE)
    p3, p2, offsets = _pack_batch([correspondences[n] for n in names])
    x0 = np.stack([_params10(cameras[n]) for n in names])
    up = lambda x: engine.upload_f64(x, dev)  # noqa: E731
    out = engine.refine_cameras(up(p3), up(p2), offsets, up(x0), n_params=10 if optimize_intrinsics else 6, f_scale=f_scale,
                                max_steps=max_steps)
    params, status, n_acc, n_trial, cost0, cost, g = (t.cpu().numpy() for t in out)
    refined, stats = {}, {}
    for c, name in enumerate(names):
        cam, (pts_3d, pts_2d) = cameras[name], correspondences[name]
        n_pts, st = int(offsets[c + 1] - offsets[c]), int(status[c])
        if st == _lib.REFINE_SKIPPED:
            if verbose:
                print(f"  {name}: too few points ({n_pts}), skipping")
            refined[name], stats[name] = cam, {"status": "skipped", "n_points": n_pts}
            continue
        if st == _lib.REFINE_NONFINITE:
            refined[name], stats[name] = cam, {"status": "non_finite", "n_points": n_pts, "n_evaluations": int(n_trial[c])}
            continue
        n_p = 10 if optimize_intrinsics else 6
        pts_3d, pts_2d = np.asarray(pts_3d, np.float64), np.asarray(pts_2d, np.float64)
        res0 = reprojection_residuals(x0[c, :n_p], pts_3d, pts_2d, cam, optimize_intrinsics)
        res1 = reprojection_residuals(params[c, :n_p], pts_3d, pts_2d, cam, optimize_intrinsics)
        refined[name] = unpack_params(params[c, :n_p], cam, optimize_intrinsics)
        s = {"status": _STATUS[st], "n_points": n_pts, "n_evaluations": int(n_trial[c])}
        s.update(_error_stats(res0, res1))
        s.update(cost_initial=float(cost0[c]), cost_final=float(cost[c]), n_accepted=int(n_acc[c]), gradient=g[c, :n_p].copy())
        stats[name] = s
        if verbose:
            print(f"  {name}: {n_pts:,d} pts | median {s['median_err_before']:.2f} -> {s['median_err_after']:.2f} px | "
                  f"<5px {s['pct_under_5px_before']:.1f}% -> {s['pct_under_5px_after']:.1f}% | "
                  f"<10px {s['pct_under_10px_before']:.1f}% -> {s['pct_under_10px_after']:.1f}%")
    return refined, stats


def optimize_camera(cam_name: str, cam: dict, pts_3d: np.ndarray, pts_2d: np.ndarray, optimize_intrinsics: bool = True,
                    verbose: bool = True, f_scale: float = 5.0, max_steps: int = 100, device=None) -> Tuple[dict, dict]:
    """One camera's parameters against its correspondences (:171-226): ``(refined_cam, stats)``."""
    refined, stats = optimize_cameras({cam_name: cam}, {cam_name: (pts_3d, pts_2d)}, optimize_intrinsics, verbose, f_scale, max_steps,
                                      device)
    return refined[cam_name], stats[cam_name]


def quick_reproj_stats(tracks_3d: np.ndarray, all_coords: Dict[str, np.ndarray], all_scores: Dict[str, np.ndarray],
                       cameras: Dict[str, dict], confidence_threshold: float = 0.3, max_points_per_cam: int = 50000) -> dict:
    """Reprojection statistics over all cameras (:260-309): median, mean, share under 5 and 10 px, number of comparisons."""
    kp_3d = tracks_3d[:, 0]
    valid_3d = ~np.isnan(kp_3d).any(axis=-1) & (kp_3d != 0).any(axis=-1)
    rng = np.random.default_rng(42)
    all_errors = []
    for name in sorted(cameras.keys()):
        if name not in all_coords:
            continue
        cam = cameras[name]
        pts_3d, pts_2d = gather_correspondences(kp_3d, valid_3d, all_coords[name], all_scores[name], cam, confidence_threshold,
                                                max_points=max_points_per_cam, rng=rng)
        if len(pts_3d) == 0:
            continue
        proj = (tri.get_projection_matrix(cam) @ np.hstack([pts_3d, np.ones((pts_3d.shape[0], 1))]).T).T
        all_errors.append(np.linalg.norm(proj[:, :2] / proj[:, 2:3] - pts_2d, axis=1))
    errs = np.concatenate(all_errors) if all_errors else np.array([0.0])
    return {"median_px": float(np.median(errs)), "mean_px": float(errs.mean()), "pct_under_5px": float(100 * (errs < 5).mean()),
            "pct_under_10px": float(100 * (errs < 10).mean()), "n_comparisons": len(errs)}


def refine_cameras(cameras: Dict[str, dict], all_coords: Dict[str, np.ndarray], all_scores: Dict[str, np.ndarray],
                   confidence_threshold: float = 0.3, min_views: int = 3, reproj_threshold: float = 15.0,
                   max_points_per_cam: int = 200000, subsample_frames: int = 5000, iterations: int = 5,
                   convergence_threshold: float = 0.05, optimize_intrinsics: bool = True, verbose: bool = False, f_scale: float = 5.0,
                   max_steps: int = 100, device=None) -> Tuple[Dict[str, dict], List[dict]]:
    """The alternation of the reference's ``main()`` (:406-562) on arrays: per iteration triangulate (RANSAC, undistorted) with the
    current cameras on the seeded frame subsample, gather every camera's correspondences, fit all cameras in one launch, triangulate
    again and measure.  Stops when the median reprojection error moves by less than ``convergence_threshold`` between iterations.
    Returns the refined cameras and one dict per iteration: ``iteration, pre, post`` (``quick_reproj_stats``), ``cameras`` (the
    per-camera stats) and ``converged``."""
    n_frames_total = max(c.shape[0] for c in all_coords.values())
    n_keypoints = list(all_coords.values())[0].shape[1]
    rng = np.random.default_rng(42)
    n_sub = min(subsample_frames, n_frames_total)
    sub_idx = np.sort(rng.choice(n_frames_total, n_sub, replace=False))
    sub_coords, sub_scores = {}, {}
    for name in all_coords:
        c, s = all_coords[name], all_scores[name]
        sub_c = np.full((n_sub, n_keypoints, 2), np.nan, dtype=np.float64)
        sub_s = np.full((n_sub, n_keypoints), np.nan, dtype=np.float64)
        mask = sub_idx < c.shape[0]
        sub_c[mask], sub_s[mask] = c[sub_idx[mask]], s[sub_idx[mask]]
        sub_coords[name], sub_scores[name] = sub_c, sub_s
    tri_kw = dict(n_frames=n_frames_total, n_keypoints=n_keypoints, confidence_threshold=confidence_threshold, min_views=min_views,
                  reproj_threshold=reproj_threshold, undistort=True, use_ransac=True, frame_indices=sub_idx, device=device)

    current = copy.deepcopy(cameras)
    history: List[dict] = []
    prev_median = None
    for iteration in range(1, iterations + 1):
        tracks_3d, _ = tri.triangulate_all(current, all_coords, all_scores, verbose=verbose, **tri_kw)
        kp_3d = tracks_3d[:, 0]
        valid_3d = ~np.isnan(kp_3d).any(axis=-1) & (kp_3d != 0).any(axis=-1)
        pre = quick_reproj_stats(tracks_3d, sub_coords, sub_scores, current, confidence_threshold, max_points_per_cam=max_points_per_cam)
        cam_rng = np.random.default_rng(42 + iteration)
        corr = {}
        for name in sorted(current.keys()):
            if name in sub_coords:
                corr[name] = gather_correspondences(kp_3d, valid_3d, sub_coords[name], sub_scores[name], current[name],
                                                    confidence_threshold=confidence_threshold, max_points=max_points_per_cam, rng=cam_rng)
        refined, cam_stats = optimize_cameras(current, corr, optimize_intrinsics, verbose, f_scale, max_steps, device)
        for name, st in cam_stats.items():
            if st["status"] not in ("skipped", "non_finite"):
                current[name] = refined[name]
        tracks_post, _ = tri.triangulate_all(current, all_coords, all_scores, verbose=False, **tri_kw)
        post = quick_reproj_stats(tracks_post, sub_coords, sub_scores, current, confidence_threshold, max_points_per_cam=max_points_per_cam)
        entry = dict(iteration=iteration, pre=pre, post=post, cameras=cam_stats, converged=False)
        history.append(entry)
        median = post["median_px"]
        if prev_median is not None and abs(prev_median - median) < convergence_threshold:
            entry["converged"] = True
            break
        prev_median = median
    return current, history
