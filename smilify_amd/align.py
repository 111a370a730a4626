"""Rigid and similarity alignment of 3-D keypoint sets on the GPU: which rotation ``R``, translation ``t`` and scale ``s`` carry
``src`` onto ``dst``, ``dst_i ~ s R src_i + t``, in the weighted least-squares sense.  It relates the 3-D keypoints that
``triangulate``, ``refine_points`` and ``bundle_adjust_alternating`` produce to a model's joints: a starting global pose for a fitter
(``global_pose_from_alignment``), the aligned joint error PA-MPJPE next to MPJPE (``joint_errors``, ``mpjpe``, ``pa_mpjpe``) for a
whole batch without a host round trip, and an alignment a regressor can be trained through.  An extension: the reference has no
alignment; only the masking rule of its MPJPE is mirrored (smal_fitter/neuralSMIL/benchmark_model.py:287-297).

The solve is Horn's quaternion method on HIP kernels (csrc/align.hip, csrc/align.h; the formulas are stated at include/smilfit.h):
no SVD, and a reflection cannot come out - a mirrored target still gets a proper rotation.  The gradient is a closed form, first
order only.  Tensors are float32 or float64 on the GPU; the arithmetic is float64 either way.  There is no CPU path: a CPU tensor
raises.  Every sum has a fixed order: the same inputs give the same bits, values and gradients, on every call.

Inputs that do not determine a rotation are reported, not guessed at.  ``status`` per problem is ``OK``; ``DEGENERATE`` for one point,
two points, collinear or coincident points (the two largest eigenvalues of Horn's matrix agree within ``min_gap``, relatively):
``R = I``, ``s = 1``, ``t`` the difference of the means; or ``EMPTY`` when no joint carries weight: the identity.  The gradients of a
problem that is not ``OK`` are exactly zero.  ``status`` is a device tensor: no call here waits for the device, except that passing
``weights`` costs one synchronisation for the check of their values (``validate_weights=False`` skips it; the kernels count a weight
that is not a positive finite number as 0)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib, engine, rotations
from .keypoint_losses import _bytes, _flags, _float_tensor, _on_gpu, _shape

OK, DEGENERATE, EMPTY = _lib.ALIGN_OK, _lib.ALIGN_DEGENERATE, _lib.ALIGN_EMPTY


class Alignment(NamedTuple):
    """``dst ~ s R src + t``: R (B,3,3), t (B,3), s (B), status (B) int32 (``OK``, ``DEGENERATE``, ``EMPTY``), gap (B) the relative gap of
    the two largest eigenvalues of Horn's matrix, rms (B) the weighted root mean square residual.  Unbatched input: no B axis."""
    R: torch.Tensor
    t: torch.Tensor
    s: torch.Tensor
    status: torch.Tensor
    gap: torch.Tensor
    rms: torch.Tensor


class _Align(torch.autograd.Function):
    """(R, t, s, status, gap, rms, final weights); the gradients on R, t and s go to src and dst."""

    @staticmethod
    def forward(ctx, src, dst, weights, mask, with_scale, min_gap, robust_iters, robust_scale):
        R, t, s, status, gap, rms, w_final, saved = engine.align_forward(src, dst, weights, mask, with_scale, min_gap, robust_iters, robust_scale)
        ctx.save_for_backward(src, dst, w_final, saved, status)
        ctx.with_scale = with_scale
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(status, gap, rms, w_final)
        return R, t, s, status, gap, rms, w_final

    @staticmethod
    @once_differentiable
    def backward(ctx, gR, gt, gs, _status, _gap, _rms, _w):
        src, dst, w_final, saved, status = ctx.saved_tensors
        c = lambda g: None if g is None else g.contiguous()  # noqa: E731
        dsrc, ddst = engine.align_backward(src, dst, w_final, saved, status, c(gR), c(gt), c(gs), ctx.with_scale, ctx.needs_input_grad[:2])
        return dsrc, ddst, None, None, None, None, None, None


def _nonneg(who: str, name: str, v, positive: bool = False) -> float:
    v = float(v)
    if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
        raise ValueError(f"{who}: {name} must be finite and {'positive' if positive else 'not negative'}, got {v}")
    return v


def _points(who: str, name: str, x, dtype=None):
    """A (B,J,3) view of a (B,J,3) or (J,3) point set and whether it was unbatched."""
    x = _float_tensor(who, name, x, dtype)
    if x.dim() not in (2, 3) or x.shape[-1] != 3:
        raise ValueError(f"{who}: {name} must be (B, J, 3) or (J, 3), got {tuple(x.shape)}")
    return (x[None], True) if x.dim() == 2 else (x, False)


def similarity_transform(src: torch.Tensor, dst: torch.Tensor, weights: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                         with_scale: bool = True, min_gap: float = 1e-10, robust_iters: int = 0, robust_scale: Optional[float] = None, *,
                         return_weights: bool = False, validate_weights: bool = True):
    """The ``Alignment`` that carries ``src`` onto ``dst``, both (B,J,3) or (J,3), minimising ``sum_i w_i |s R src_i + t - dst_i|^2``.

    ``weights`` (J) or (B,J), ``>= 0`` and finite, times ``mask`` (B,J) (bool or any numeric type, non-zero: true) is the weight of a
    joint; it is 0 where a coordinate of either point is not finite, and a joint of weight 0 is not read.  ``with_scale=False``
    fixes ``s = 1`` (``rigid_transform``).  ``min_gap``: the relative eigenvalue gap at or below which a problem is ``DEGENERATE``.

    ``robust_iters > 0`` re-solves that many times with ``w_i = w0_i / sqrt(1 + r_i^2 / robust_scale^2)``, ``r_i`` the residual of
    joint i under the solve before - soft-L1, the cost of ``refine_points``; outliers further than a few ``robust_scale`` lose their
    say.  The result is that of the last solve, and the gradient treats its weights as constants: it is the gradient of the
    weighted solve at the final weights, not of the iteration.  ``return_weights=True`` returns ``(Alignment, weights (B,J)
    float64)``, the weights of the last solve.

    Gradients go to ``src`` and ``dst`` from ``R``, ``t`` and ``s``; ``status``, ``gap`` and ``rms`` carry none, and neither do the
    weights or the mask."""
    who = "similarity_transform" if with_scale else "rigid_transform"
    src, unbatched = _points(who, "src", src)
    dst, dst_unbatched = _points(who, "dst", dst, src.dtype)
    if unbatched != dst_unbatched:
        raise ValueError(f"{who}: src and dst must both be (B, J, 3) or both (J, 3)")
    _shape(who, "dst", dst, src.shape)
    B, J = int(src.shape[0]), int(src.shape[1])
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype.is_complex or weights.dtype == torch.bool or \
                tuple(weights.shape) not in ((J,), (B, J)):
            raise ValueError(f"{who}: weights must be a real tensor of shape ({J},) or ({B}, {J}), got {tuple(getattr(weights, 'shape', ()))}")
        if unbatched and weights.dim() == 2:
            raise ValueError(f"{who}: unbatched points take weights of shape ({J},)")
    mask = _flags(who, "mask", None if mask is None else (mask[None] if unbatched and isinstance(mask, torch.Tensor) else mask), (B, J))
    min_gap = _nonneg(who, "min_gap", min_gap)
    robust_iters = int(robust_iters)
    if robust_iters < 0:
        raise ValueError(f"{who}: robust_iters must not be negative, got {robust_iters}")
    if robust_iters > 0 and robust_scale is None:
        raise ValueError(f"{who}: robust_iters > 0 needs a robust_scale")
    robust_scale = 1.0 if robust_scale is None else _nonneg(who, "robust_scale", robust_scale, positive=True)
    if weights is not None and validate_weights and weights.numel() > 0:
        w = weights.detach()
        if not bool((torch.isfinite(w) & (w >= 0)).all()):  # (the one read of device memory: see the module's docstring)
            raise ValueError(f"{who}: weights must be finite and not negative")
    device = _on_gpu(src, dst, weights, mask)
    w64 = None if weights is None else weights.detach().to(torch.float64).contiguous()
    R, t, s, status, gap, rms, w_final = _Align.apply(src.contiguous(), dst.contiguous(), w64, _bytes(mask, device), bool(with_scale), min_gap,
                                                      robust_iters, robust_scale)
    out = Alignment(R, t, s, status, gap, rms)
    if unbatched:
        out, w_final = Alignment(*(v[0] for v in out)), w_final[0]
    return (out, w_final) if return_weights else out


def rigid_transform(src: torch.Tensor, dst: torch.Tensor, weights: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                    min_gap: float = 1e-10, robust_iters: int = 0, robust_scale: Optional[float] = None, **kw):
    """``similarity_transform`` with ``with_scale=False``: rotation and translation only, ``s = 1``."""
    return similarity_transform(src, dst, weights, mask, False, min_gap, robust_iters, robust_scale, **kw)


def apply_transform(points: torch.Tensor, R: torch.Tensor, t: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """``s R p + t`` for points (..., P, 3) under R (..., 3, 3), t (..., 3), s (...): plain torch operations, differentiable in all."""
    return s[..., None, None] * (points @ R.transpose(-1, -2)) + t[..., None, :]


def joint_errors(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, align: str = "none", sentinel: bool = True,
                 scale: float = 1.0, min_gap: float = 1e-10):
    """Per-joint errors of ``pred`` against ``target``, both (B,J,3) or (J,3), in one kernel: ``(dist (B,J), valid (B,J) bool, status (B)
    int32)``.  A joint is valid where ``mask`` (B,J) is non-zero, both points are finite and, with ``sentinel``, ``|target| > 1e-6``
    (the reference's "no annotation" rule).  ``align``: ``"none"`` (MPJPE), or ``"rigid"`` / ``"similarity"``: the alignment that carries
    ``pred`` onto ``target`` with ``valid`` as weights is applied first (PA-MPJPE).  ``dist = scale |aligned pred - target|``, 0 where
    the joint is not valid (``scale``: the reference's ``1 / world_scale``, back to millimetres).  A sample whose valid joints do not
    determine a rotation uses its fall-back transform and says so in ``status``.  Forward only: no gradient."""
    who = "joint_errors"
    if align not in engine.ALIGN_MODES:
        raise ValueError(f"{who}: align must be one of {tuple(engine.ALIGN_MODES)}, got {align!r}")
    pred, unbatched = _points(who, "pred", pred)
    target, target_unbatched = _points(who, "target", target, pred.dtype)
    if unbatched != target_unbatched:
        raise ValueError(f"{who}: pred and target must both be (B, J, 3) or both (J, 3)")
    _shape(who, "target", target, pred.shape)
    mask = _flags(who, "mask", None if mask is None else (mask[None] if unbatched and isinstance(mask, torch.Tensor) else mask),
                  tuple(pred.shape[:2]))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"{who}: scale must be finite, got {scale}")
    min_gap = _nonneg(who, "min_gap", min_gap)
    device = _on_gpu(pred, target, mask)
    dist, valid, status = engine.align_errors(pred.detach().contiguous(), target.detach().contiguous(), _bytes(mask, device),
                                              engine.ALIGN_MODES[align], sentinel, scale, min_gap)
    valid = valid.bool()
    return (dist[0], valid[0], status[0]) if unbatched else (dist, valid, status)


def _pooled(dist: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    # the reference pools every valid joint of the batch (benchmark_model.py:296-298); float64 sum of (B,J) values, on the device
    return (dist.double().sum() / valid.sum().clamp(min=1)).to(dist.dtype)


def mpjpe(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, sentinel: bool = True,
          scale: float = 1.0) -> torch.Tensor:
    """The mean per-joint position error over every valid joint of the batch, ``dist.sum() / valid.sum()`` of ``joint_errors`` without
    alignment, as a 0-dim device tensor; 0 for a batch with nothing valid."""
    dist, valid, _ = joint_errors(pred, target, mask, "none", sentinel, scale)
    return _pooled(dist, valid)


def pa_mpjpe(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, with_scale: bool = True, sentinel: bool = True,
             scale: float = 1.0, min_gap: float = 1e-10) -> torch.Tensor:
    """``mpjpe`` after each sample's prediction has been aligned to its target (similarity, or rigid with ``with_scale=False``)."""
    dist, valid, _ = joint_errors(pred, target, mask, "similarity" if with_scale else "rigid", sentinel, scale, min_gap)
    return _pooled(dist, valid)


def global_pose_from_alignment(smal, R: torch.Tensor, t: torch.Tensor, beta: Optional[torch.Tensor] = None, *,
                               root: Optional[torch.Tensor] = None, global_rotation: Optional[torch.Tensor] = None,
                               trans: Optional[torch.Tensor] = None):
    """The global-rotation row and ``trans`` that move a model by a rigid alignment of its joints.

    ``R`` (B,3,3), ``t`` (B,3): ``rigid_transform(joints, target)`` of the joints ``smal`` (a ``SMAL``) returned for some pose.  That
    pose had the global rotation ``global_rotation`` (B,3) axis-angle and the translation ``trans`` (B,3); both default to zero.
    Returns ``(global_rotation (B,3) axis-angle, trans (B,3))`` in float32, ready to replace row 0 of ``theta`` and ``trans``: posed
    with them the model's joints AND vertices are the old ones under ``p -> R p + t``.

    The convention is that of this library's LBS (csrc/lbs.hip, csrc/skin.h): the global rotation ``G`` turns the body about its root
    joint ``c`` - the root's world transform is ``[G | c]``, and the root is neither scaled nor moved by ``betas_logscale`` /
    ``betas_trans`` - and ``trans`` is added afterwards (``trans_after_joints``; ``SMAL.__call__`` regresses the joints from the
    translated vertices, the same thing for a regressor whose columns sum to 1): ``p = G (p0 - c) + c + trans``.  So
    ``R p + t = (R G) (p0 - c) + c + [R (c + trans) + t - c]``.

    ``c`` is the rest-pose root joint: of the template shaped by ``beta`` (B,nB) or (nB) (``None``: the template itself), or ``root``
    (B,3) / (3) given directly - ``smal.J_transformed[:, 0]`` after any call - for a model called with ``del_v`` or ``v_template``."""
    who = "global_pose_from_alignment"
    R = _float_tensor(who, "R", R)
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3):
        raise ValueError(f"{who}: R must be (B, 3, 3), got {tuple(R.shape)}")
    B = int(R.shape[0])
    t = _float_tensor(who, "t", t, R.dtype)
    _shape(who, "t", t, (B, 3))
    device = _on_gpu(R, t)
    f64 = lambda x: x.detach().to(device=device, dtype=torch.float64)  # noqa: E731
    if root is not None:
        c = f64(root).expand(B, 3)
    else:
        tab = smal.tables
        if tab.static_joints:
            c = torch.from_numpy(tab.J_static[0]).to(device=device, dtype=torch.float64).expand(B, 3)
        else:
            col = f64(smal.J_regressor)[:, 0]  # (V): the root's row of the regressor
            c = (col @ f64(smal.v_template)).expand(B, 3)
            if beta is not None and beta.shape[-1] > 0:
                nB = int(beta.shape[-1])
                dirs = f64(smal.shapedirs)[:nB].reshape(nB, -1, 3)  # (nB,V,3)
                c = c + f64(beta).reshape(-1, nB).expand(B, nB) @ torch.einsum("v,kvd->kd", col, dirs)
    R64, shift = f64(R), c
    if trans is not None:
        shift = c + f64(trans).expand(B, 3)
    new_trans = (R64 @ shift[..., None])[..., 0] + f64(t) - c
    if global_rotation is not None:
        R64 = R64 @ rotations.axis_angle_to_matrix(f64(global_rotation).expand(B, 3).contiguous())
    return rotations.matrix_to_axis_angle(R64.contiguous()).float(), new_trans.float()
