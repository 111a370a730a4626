"""Robust nonlinear refinement of triangulated points on the HIP kernel (``csrc/refine_points.hip``), and the block-coordinate bundle
adjustment it makes with the camera refinement (``csrc/refine.hip``).

AN EXTENSION: the reference has no such function.  Its points stay the DLT points of ``triangulate_point_dlt``, which minimise an
algebraic error; here every point is moved from the DLT point to the minimum of the cost the cameras are fitted with (scipy's
``soft_l1`` on every scalar reprojection residual, ``f_scale`` 5 px) over the views of its final system.  Everything is float64, numpy
in and numpy out, and there is no CPU path for the fit.  Deviations from what a scipy user would write:

* the optimiser is the Levenberg-Marquardt of ``refine_cameras`` in three unknowns, not scipy's trust-region-reflective: same cost,
  same minimum, other iterates;
* the Jacobian is analytic;
* a soft_l1 cost with outliers can have several minima: the result is the one the descent from ``xyz0`` reaches.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib, engine
from . import refine_cameras as rc
from . import triangulate as tri

__all__ = ["refine_points_arrays", "evaluate_points_cost", "observation_costs", "view_bits", "bundle_adjust_alternating"]

STATUS_NAMES = {_lib.REFINE_CONVERGED: "converged", _lib.REFINE_STEP_LIMIT: "step_limit", _lib.REFINE_POINTS_FEW_VIEWS: "few_views",
                _lib.REFINE_NONFINITE: "non_finite"}


def _upload(P, obs, view_mask, xyz, device):
    dev = engine.require_gpu(device or tri.DEFAULT_DEVICE)
    obs = np.asarray(obs, np.float64)
    if obs.ndim != 4 or obs.shape[3] != 2:
        raise ValueError("refine_points: obs must be (N, Kp, C, 2)")
    if obs.shape[2] > _lib.TRI_MAX_VIEWS:
        raise ValueError(f"refine_points: {obs.shape[2]} cameras above SMIL_TRI_MAX_VIEWS={_lib.TRI_MAX_VIEWS}")
    up = lambda x: engine.upload_f64(x, dev)  # noqa: E731
    mask = np.ascontiguousarray(np.asarray(view_mask).astype(np.uint32, copy=False)).view(np.int32)
    return up(np.asarray(P, np.float64).reshape(-1, 3, 4)), up(obs), torch.from_numpy(mask.copy()).to(dev), up(xyz)


def refine_points_arrays(P, obs, view_mask, xyz0, f_scale: float = 5.0, max_steps: int = 50, device=None) -> Tuple[np.ndarray, dict]:
    """Every point of xyz0 (N,Kp,3) moved to the minimum of the soft_l1 reprojection cost over the views of view_mask (N,Kp) uint32
    (bit c = camera c) of obs (N,Kp,C,2), undistorted pixels, through P (C,3,4): the layouts ``triangulate_arrays`` returns as
    ``obs_undistorted``, ``inlier_mask`` and ``xyz``.  Returns ``(xyz (N,Kp,3), stats)``; stats holds ``status`` (0 converged, 1 step
    limit, 2 fewer than two views, 3 non-finite cost at xyz0; 2 and 3 return the point unchanged), ``n_accepted``, ``n_trials``,
    ``cost_initial``, ``cost_final`` (N,Kp) and ``view_err`` (N,Kp,C): the reprojection error at the returned point, NaN outside the
    mask."""
    out = engine.refine_points(*_upload(P, obs, view_mask, xyz0, device), f_scale=f_scale, max_steps=max_steps, want_view_err=True)
    xyz, status, n_acc, n_trial, cost0, cost, view_err = (t.cpu().numpy() for t in out)
    return xyz, dict(status=status, n_accepted=n_acc, n_trials=n_trial, cost_initial=cost0, cost_final=cost, view_err=view_err)


def evaluate_points_cost(P, obs, view_mask, xyz, f_scale: float = 5.0, device=None):
    """One accumulation of the kernel at xyz (N,Kp,3): ``cost (N,Kp), g (N,Kp,3), H (N,Kp,3,3)`` as numpy (no view: zeros)."""
    out = engine.refine_points_evaluate(*_upload(P, obs, view_mask, xyz, device), f_scale=f_scale)
    return tuple(t.cpu().numpy() for t in out)


def view_bits(view_mask, C: int) -> np.ndarray:
    """(..., C) bool: bit c of every mask."""
    return ((np.asarray(view_mask).astype(np.uint32)[..., None] >> np.arange(C, dtype=np.uint32)) & np.uint32(1)).astype(bool)


def observation_costs(P, obs, view_mask, xyz, f_scale: float = 5.0) -> np.ndarray:
    """The soft_l1 cost of every scalar residual on the host, (N,Kp,C,2) float64, exactly zero outside the mask: summed over the last two
    axes it is the cost of a point, summed over the first two and the last that of a camera, and either way the same total."""
    P, obs, xyz = np.asarray(P, np.float64).reshape(-1, 3, 4), np.asarray(obs, np.float64), np.asarray(xyz, np.float64)
    with np.errstate(all="ignore"):
        h = np.einsum("cij,nkj->nkci", P[:, :, :3], xyz) + P[:, :, 3]
        z = ((h[..., :2] / h[..., 2:3] - obs) / f_scale) ** 2
        rho = 0.5 * f_scale ** 2 * (2.0 * z / (np.sqrt(1.0 + z) + 1.0))
    return np.where(view_bits(view_mask, len(P))[..., None], rho, 0.0)


def _projection(params10: np.ndarray) -> np.ndarray:
    """K [R | t] of a parameter row (rvec, t, fx, fy, cx, cy): the pinhole model the camera half fits (no skew)."""
    p = np.asarray(params10, np.float64)
    K = np.array([[p[6], 0.0, p[8]], [0.0, p[7], p[9]], [0.0, 0.0, 1.0]])
    return K @ np.hstack([rc.rodrigues(p[:3]), p[3:6].reshape(3, 1)])


def bundle_adjust_alternating(cameras: Dict[str, dict], obs, view_mask, xyz0, iterations: int = 5, optimize_intrinsics: bool = True,
                              f_scale: float = 5.0, max_steps_points: int = 50, max_steps_cameras: int = 100,
                              device=None) -> Tuple[Dict[str, dict], np.ndarray, List[dict]]:
    """Block-coordinate descent on ONE robust cost over a FIXED observation set: per iteration one ``refine_points_arrays`` (cameras
    held) followed by one ``optimize_cameras`` (points held) over the same observations.  Unlike ``refine_cameras`` there is no
    re-triangulation, no subsampling and no 20-correspondence skip rule, so neither half can raise the total.

    ``cameras``: name -> {K, R or rvec, t}; axis C of obs (N,Kp,C,2), undistorted pixels, follows ``sorted(cameras)``.  The observation
    set is the bits of view_mask (N,Kp) of the points that have at least two views and a finite xyz0; the other points are returned
    as they came and take no part.  A camera that sees fewer than 20 points is held fixed (the kernel's SMIL_REFINE_MIN_POINTS); its
    observations still count in the cost and its name is listed under ``held_fixed``.  The cameras are the 10-parameter pinhole model
    of ``refine_cameras.pack_params``: a skew entry of K is not carried.

    Returns ``(cameras, xyz, history)``.  history has one dict per half step, after a first one for the start: ``iteration``,
    ``half`` ("start", "points" or "cameras"), ``total`` (the soft_l1 cost over all masked observations, summed by point from the
    point kernel), ``total_by_camera`` (the same state summed by camera from the camera kernel), and for the camera half ``cameras``
    (the per-camera stats) and ``held_fixed``; for the point half ``status_counts``."""
    names = sorted(cameras)
    obs, xyz = np.asarray(obs, np.float64), np.array(xyz0, np.float64)
    C = len(names)
    if obs.ndim != 4 or obs.shape[2:] != (C, 2) or xyz.shape != obs.shape[:2] + (3,):
        raise ValueError("bundle_adjust_alternating: obs must be (N, Kp, len(cameras), 2) and xyz0 (N, Kp, 3)")
    bits = view_bits(view_mask, C)
    bits &= ((bits.sum(-1) >= 2) & np.isfinite(xyz).all(-1))[..., None]
    mask = (bits.astype(np.uint32) << np.arange(C, dtype=np.uint32)).sum(-1).astype(np.uint32)
    current = {n: rc.unpack_params(rc.pack_params(cameras[n], True), cameras[n], True) for n in names}
    where = [np.nonzero(bits[..., c]) for c in range(C)]

    def state():
        params = np.stack([rc.pack_params(current[n], True) for n in names])
        P = np.stack([_projection(p) for p in params])
        corr = {n: (xyz[where[c]], obs[where[c]][:, c]) for c, n in enumerate(names)}
        return params, P, corr

    def totals(params, P, corr):
        by_point = evaluate_points_cost(P, obs, mask, xyz, f_scale, device)[0]
        by_camera = rc.evaluate_cost(params, [corr[n] for n in names], optimize_intrinsics, f_scale, device)[0]
        return dict(total=float(by_point.sum()), total_by_camera=float(by_camera.sum()))

    params, P, corr = state()
    history: List[dict] = [dict(iteration=0, half="start", **totals(params, P, corr))]
    for iteration in range(1, iterations + 1):
        new, st = refine_points_arrays(P, obs, mask, xyz, f_scale, max_steps_points, device)
        moved = (st["status"] == _lib.REFINE_CONVERGED) | (st["status"] == _lib.REFINE_STEP_LIMIT)
        xyz[moved] = new[moved]
        params, P, corr = state()
        counts = {STATUS_NAMES[k]: int((st["status"] == k).sum()) for k in STATUS_NAMES}
        history.append(dict(iteration=iteration, half="points", status_counts=counts, **totals(params, P, corr)))

        refined, cam_stats = rc.optimize_cameras(current, corr, optimize_intrinsics, False, f_scale, max_steps_cameras, device)
        held = [n for n in names if cam_stats[n]["status"] in ("skipped", "non_finite")]
        for n in names:
            if n not in held:
                current[n] = refined[n]
        params, P, corr = state()
        history.append(dict(iteration=iteration, half="cameras", cameras=cam_stats, held_fixed=held, **totals(params, P, corr)))
    return copy.deepcopy(current), xyz, history
