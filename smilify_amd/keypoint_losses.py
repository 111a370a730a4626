"""The geometry half of a multi-view regressor's loss head on the GPU: 2-D and 3-D keypoint losses, projection of predicted joints
through predicted per-view cameras, the two fused, and the triangulation-consistency term (reference
smal_fitter/neuralSMIL/multiview_smil_regressor.py:1050-1110, :1623-1838, :2250-2388 and the per-sample loops of
smil_image_regressor.py:3032-3115, :3334-3407).  Unlike ``Renderer`` / ``CameraSet``, whose ``R`` and ``T`` are constants, every
function here sends gradients to ``R``, ``T`` and ``fov``, so camera heads can be trained through it.

Every function is a ``torch.autograd.Function`` over forward and analytic backward HIP kernels (csrc/keypoint_losses.hip; the
formulas are stated at include/smilfit.h).  Tensors are float32 or float64 on the GPU; the arithmetic is float64 either way.
First-order gradients only.  There is no CPU path: a CPU tensor raises - visibility, masks and joint weights included, nothing is
copied to the device behind the caller's back.  No call synchronises with the host, and every sum has a fixed order: the same
inputs give the same bits, values and gradients, on every call.

Visibility and masks may be bool, uint8 or any integer or floating type; non-zero means true.  Camera arguments are stacked tensors
``R (B,V,3,3)``, ``T (B,V,3)``, ``fov (B,V)`` (degrees; ``(B,V,1)`` is accepted), ``aspect_ratio (B,V)``, or the reference's
per-view lists of ``(B,3,3)``, ``(B,3)``, ``(B,1)`` / ``(B,)`` tensors.  Keypoints are normalised ``(y, x)`` in [0,1].

Deliberately not reproduced: the multi-view 3-D term's ``|t| > 1e-6`` variant of the all-zero sentinel test (here: ``sum |t| > 0``,
as the single-view loss), the reference's ``isfinite(loss)`` fall-backs to a constant (the caller's business: a non-finite loss is
returned as it is) and its warning prints."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib, engine

EPS = 1e-8


# ---- argument checks: shapes and dtypes first (ValueError), then the device (SmilError) ------------------------------------------
def _float_tensor(who: str, name: str, x, dtype=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype not in engine.ROT_DTYPES:
        raise ValueError(f"{who}: {name} must be float32 or float64, got {x.dtype}")
    if dtype is not None and x.dtype != dtype:
        raise ValueError(f"{who}: {name} is {x.dtype}, expected {dtype} like the first argument")
    return x


def _shape(who: str, name: str, x: torch.Tensor, shape) -> None:
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {tuple(shape)}, got {tuple(x.shape)}")


def _flags(who: str, name: str, x, shape) -> Optional[torch.Tensor]:
    """A visibility / mask argument of any numeric type, checked against ``shape`` (conversion happens on the device, later)."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype.is_complex:
        raise ValueError(f"{who}: {name} must be bool, integer or floating, got {x.dtype}")
    _shape(who, name, x, shape)
    return x


def _bytes(x: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """non-zero -> 1 as contiguous uint8 (``x`` is on ``device`` already: ``_on_gpu`` saw it)"""
    if x is None:
        return None
    x = x.detach()
    return (x if x.dtype == torch.bool else x != 0).contiguous().view(torch.uint8)


def _weights(who: str, w, J: int) -> Optional[torch.Tensor]:
    if w is None:
        return None
    if not isinstance(w, torch.Tensor) or w.dtype.is_complex or tuple(w.shape) != (J,):
        raise ValueError(f"{who}: joint_weights must be a real tensor of shape ({J},), got {tuple(getattr(w, 'shape', ()))}")
    return w


def _weights_f64(w: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    return None if w is None else w.detach().to(dtype=torch.float64).contiguous()  # (on ``device`` already: ``_on_gpu`` saw it)


def _on_gpu(*tensors) -> torch.device:
    device = None
    for t in tensors:
        if t is None:
            continue
        engine.require_gpu(t.device)
        if device is not None and t.device != device:
            raise _lib.SmilError(f"tensors on different devices: {device} and {t.device}")
        device = t.device
    return device


def _stacked(who: str, name: str, x, tail, squeeze_last: bool = False):
    """A camera argument as a stacked (B,V,*tail) tensor: a per-view list of (B,*tail) tensors is stacked along a new axis 1."""
    if isinstance(x, (list, tuple)):
        if len(x) == 0:
            raise ValueError(f"{who}: {name} is an empty list")
        views = []
        for i, t in enumerate(x):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name}[{i}] must be a torch.Tensor, got {type(t).__name__}")
            if squeeze_last and t.dim() == 2 and t.shape[-1] == 1:
                t = t.squeeze(-1)
            views.append(t)
        if any(v.shape != views[0].shape for v in views):
            raise ValueError(f"{who}: the tensors of {name} differ in shape")
        x = torch.stack(views, dim=1)
    elif isinstance(x, torch.Tensor) and squeeze_last and x.dim() == 3 and x.shape[-1] == 1:
        x = x.squeeze(-1)
    if not isinstance(x, torch.Tensor) or x.dim() != 2 + len(tail) or tuple(x.shape[2:]) != tuple(tail):
        raise ValueError(f"{who}: {name} must be (B, V{''.join(', ' + str(t) for t in tail)}) or a per-view list, got "
                         f"{tuple(getattr(x, 'shape', ()))}")
    return x


def _cameras(who: str, R, T, fov, aspect, B: int, dtype):
    """Stacked, checked cameras ``(R, T, fov, aspect or None, V)`` for ``B`` samples."""
    R = _float_tensor(who, "R", _stacked(who, "R", R, (3, 3)), dtype)
    V = int(R.shape[1])
    T = _float_tensor(who, "T", _stacked(who, "T", T, (3,)), dtype)
    fov = _float_tensor(who, "fov", _stacked(who, "fov", fov, (), squeeze_last=True), dtype)
    if isinstance(aspect, (list, tuple)) and len(aspect) == 0:
        aspect = None  # (the reference's empty list: aspect 1)
    if aspect is not None:
        aspect = _float_tensor(who, "aspect_ratio", _stacked(who, "aspect_ratio", aspect, (), squeeze_last=True), dtype)
    for name, t, tail in (("R", R, (3, 3)), ("T", T, (3,)), ("fov", fov, ()), ("aspect_ratio", aspect, ())):
        if t is not None:
            _shape(who, name, t, (B, V) + tail)
    return R, T, fov, aspect, V


def _image_size(who: str, image_size) -> float:
    S = float(image_size)
    if not (S > 0.0 and S < float("inf")):
        raise ValueError(f"{who}: image_size must be positive and finite, got {image_size}")
    return S


def _c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.contiguous()


# ---- autograd functions -----------------------------------------------------------------------------------------------------------
class _SquaredError(torch.autograd.Function):
    """loss = reduction of the masked weighted squared error of pred, target (N,J,D); the gradient goes to pred."""

    @staticmethod
    def forward(ctx, pred, target, vis, mask, weights, flags, rule):
        loss, factor = engine.kp_se_forward(pred, target, vis, mask, weights, flags, rule)
        ctx.save_for_backward(pred, target, vis, mask, weights, factor)
        ctx.flags = flags
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pred, target, vis, mask, weights, factor = ctx.saved_tensors
        dpred = engine.kp_se_backward(pred, target, vis, mask, weights, factor, grad.contiguous(), ctx.flags) if ctx.needs_input_grad[0] else None
        return dpred, None, None, None, None, None, None


class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, joints, R, T, fov, aspect, S):
        ctx.save_for_backward(joints, R, T, fov, aspect)
        ctx.S = S
        return engine.kp_project(joints, R, T, fov, aspect, S)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        joints, R, T, fov, aspect = ctx.saved_tensors
        return engine.kp_project_backward(joints, R, T, fov, aspect, grad.contiguous(), ctx.S, ctx.needs_input_grad[:4]) + (None, None)


class _ProjectLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, joints, R, T, fov, aspect, target, vis, view_mask, weights, S):
        loss, factor = engine.kp_project_loss(joints, R, T, fov, aspect, target, vis, view_mask, weights, S)
        ctx.save_for_backward(joints, R, T, fov, aspect, target, vis, view_mask, weights, factor)
        ctx.S = S
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        joints, R, T, fov, aspect, target, vis, view_mask, weights, factor = ctx.saved_tensors
        grads = engine.kp_project_loss_backward(joints, R, T, fov, aspect, target, vis, view_mask, weights, factor, grad.contiguous(), ctx.S,
                                                ctx.needs_input_grad[:4])
        return grads + (None,) * 6


class _Triangulate(torch.autograd.Function):
    """(points, valid, sane); the gradient on the points goes to R, T and fov."""

    @staticmethod
    def forward(ctx, kp, vis, view_mask, R, T, fov, aspect, S, damping, max_norm):
        ctx.save_for_backward(kp, vis, view_mask, R, T, fov, aspect)
        ctx.S, ctx.damping = S, damping
        points, valid, sane = engine.kp_triangulate(kp, vis, view_mask, R, T, fov, aspect, S, damping, max_norm)
        ctx.mark_non_differentiable(valid, sane)
        return points, valid, sane

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _valid, _sane):
        kp, vis, view_mask, R, T, fov, aspect = ctx.saved_tensors
        dR, dT, dfov = engine.kp_triangulate_backward(kp, vis, view_mask, R, T, fov, aspect, grad.contiguous(), ctx.S, ctx.damping,
                                                      ctx.needs_input_grad[3:6])
        return None, None, None, dR, dT, dfov, None, None, None, None


# ---- public functions -------------------------------------------------------------------------------------------------------------
def _keypoint_loss(who, pred, target, visibility, joint_weights, mask, reduction, reductions, D, flags):
    if reduction not in reductions:
        raise ValueError(f"{who}: reduction must be one of {reductions}, got {reduction!r}")
    pred = _float_tensor(who, "the prediction", pred)
    if pred.dim() < 2 or pred.shape[-1] != D:
        raise ValueError(f"{who}: the prediction must be (..., J, {D}), got {tuple(pred.shape)}")
    target = _float_tensor(who, "target", target, pred.dtype)
    _shape(who, "target", target, pred.shape)
    lead, J = tuple(pred.shape[:-2]), int(pred.shape[-2])
    visibility = _flags(who, "visibility", visibility, lead + (J,))
    mask = _flags(who, "mask", mask, lead)
    joint_weights = _weights(who, joint_weights, J)
    device = _on_gpu(pred, target, visibility, mask, joint_weights)
    N = 1
    for s in lead:
        N *= int(s)
    return _SquaredError.apply(pred.contiguous().reshape(N, J, D), target.detach().contiguous().reshape(N, J, D),
                               None if visibility is None else _bytes(visibility, device).reshape(N, J),
                               None if mask is None else _bytes(mask, device).reshape(N), _weights_f64(joint_weights, device), flags,
                               engine.KP_REDUCTIONS[reduction])


def keypoint_loss_2d(rendered: torch.Tensor, target: torch.Tensor, visibility: Optional[torch.Tensor], *, joint_weights=None, mask=None,
                     reduction: str = "pooled") -> torch.Tensor:
    """The visibility-weighted 2-D keypoint loss of ``rendered``, ``target`` (..., J, 2) normalised to [0,1], ``visibility`` (..., J),
    optional ``joint_weights`` (J) and a ``mask`` (...) over the samples (a view mask for (B,V,J,2) input).  A joint counts where it
    is visible, its sample selected and both target coordinates lie in [0,1]; a non-finite rendered coordinate counts as 0 and gets
    no gradient.  With ``num_n``, ``count_n`` the weighted squared error and weight of sample n and eps = 1e-8:

    * ``"pooled"``: ``sum num / (2 sum count + eps) + eps`` (``_compute_batched_keypoint_loss``);
    * ``"valid_samples"``: the mean of ``num_n / (2 count_n + eps)`` over selected samples holding a valid joint, plus eps (the
      single-view per-sample loop);
    * ``"samples"``: that mean over all selected samples, plus eps (``_compute_visibility_weighted_keypoint_loss``).

    With nothing valid the value is exactly eps and the gradient exactly zero.  The gradient goes to ``rendered`` only."""
    return _keypoint_loss("keypoint_loss_2d", rendered, target, visibility, joint_weights, mask, reduction,
                          ("pooled", "valid_samples", "samples"), 2, engine.KP_FLAGS_2D)


def keypoint_loss_3d(joints: torch.Tensor, target: torch.Tensor, visibility: Optional[torch.Tensor], *, joint_weights=None, mask=None,
                     reduction: str = "valid_samples") -> torch.Tensor:
    """The 3-D keypoint loss of ``joints``, ``target`` (..., J, 3): as ``keypoint_loss_2d`` with 3 for 2, and a joint counts where it
    is visible, its sample selected, prediction and target are finite and the target is not the all-zero sentinel (``sum |t| > 0``;
    the multi-view reference's ``|t| > 1e-6`` variant is not reproduced)."""
    return _keypoint_loss("keypoint_loss_3d", joints, target, visibility, joint_weights, mask, reduction, ("valid_samples", "pooled"), 3,
                          engine.KP_FLAGS_3D)


def _joints_and_cameras(who, joints_3d, R, T, fov, aspect_ratio, image_size):
    joints_3d = _float_tensor(who, "joints_3d", joints_3d)
    if joints_3d.dim() != 3 or joints_3d.shape[-1] != 3:
        raise ValueError(f"{who}: joints_3d must be (B, J, 3), got {tuple(joints_3d.shape)}")
    R, T, fov, aspect, V = _cameras(who, R, T, fov, aspect_ratio, int(joints_3d.shape[0]), joints_3d.dtype)
    return joints_3d, R, T, fov, aspect, V, _image_size(who, image_size)


def project_joints_to_views(joints_3d: torch.Tensor, R, T, fov, image_size, aspect_ratio=None) -> torch.Tensor:
    """``joints_3d`` (B,J,3) through B x V FoV cameras -> (B,V,J,2): screen ``(y, x)`` of an ``image_size`` square image divided by
    ``image_size + 1e-8`` and clamped to [0,1] (``_batch_project_joints_to_views``; the camera of ``Renderer``, in float64).
    Gradients go to the joints, ``R`` (all nine entries), ``T`` and ``fov``; none to ``aspect_ratio``.  A clamped coordinate passes
    its gradient where the unclamped value lies in [0,1], as ``torch.clamp``."""
    who = "project_joints_to_views"
    joints_3d, R, T, fov, aspect, _, S = _joints_and_cameras(who, joints_3d, R, T, fov, aspect_ratio, image_size)
    _on_gpu(joints_3d, R, T, fov, aspect)
    return _Project.apply(joints_3d.contiguous(), R.contiguous(), T.contiguous(), fov.contiguous(), _c(None if aspect is None else aspect.detach()), S)


def multiview_keypoint_loss(joints_3d: torch.Tensor, R, T, fov, target: torch.Tensor, visibility: Optional[torch.Tensor], image_size, *,
                            aspect_ratio=None, view_mask=None, joint_weights=None) -> torch.Tensor:
    """``keypoint_loss_2d(project_joints_to_views(...), target (B,V,J,2), visibility (B,V,J), mask=view_mask (B,V),
    reduction="pooled")`` in one forward and two backward kernels; the projected array is never written."""
    who = "multiview_keypoint_loss"
    joints_3d, R, T, fov, aspect, V, S = _joints_and_cameras(who, joints_3d, R, T, fov, aspect_ratio, image_size)
    B, J = int(joints_3d.shape[0]), int(joints_3d.shape[1])
    target = _float_tensor(who, "target", target, joints_3d.dtype)
    _shape(who, "target", target, (B, V, J, 2))
    visibility = _flags(who, "visibility", visibility, (B, V, J))
    view_mask = _flags(who, "view_mask", view_mask, (B, V))
    joint_weights = _weights(who, joint_weights, J)
    device = _on_gpu(joints_3d, R, T, fov, aspect, target, visibility, view_mask, joint_weights)
    return _ProjectLoss.apply(joints_3d.contiguous(), R.contiguous(), T.contiguous(), fov.contiguous(),
                              _c(None if aspect is None else aspect.detach()), target.detach().contiguous(), _bytes(visibility, device),
                              _bytes(view_mask, device), _weights_f64(joint_weights, device), S)


def _triangulation_inputs(who, keypoints_2d, visibility, R, T, fov, aspect_ratio, view_mask, image_size, damping):
    keypoints_2d = _float_tensor(who, "keypoints_2d", keypoints_2d)
    if keypoints_2d.dim() != 4 or keypoints_2d.shape[-1] != 2:
        raise ValueError(f"{who}: keypoints_2d must be (B, V, J, 2), got {tuple(keypoints_2d.shape)}")
    B, Vk, J = (int(s) for s in keypoints_2d.shape[:3])
    R, T, fov, aspect, V = _cameras(who, R, T, fov, aspect_ratio, B, keypoints_2d.dtype)
    if V != Vk:
        raise ValueError(f"{who}: keypoints_2d holds {Vk} views, the cameras {V}")
    visibility = _flags(who, "visibility", visibility, (B, V, J))
    view_mask = _flags(who, "view_mask", view_mask, (B, V))
    damping = float(damping)
    if not (damping > 0.0 and damping < float("inf")):
        raise ValueError(f"{who}: damping must be positive and finite, got {damping}")
    return keypoints_2d, visibility, view_mask, R, T, fov, aspect, _image_size(who, image_size), damping


def triangulate_joints_dlt(keypoints_2d: torch.Tensor, visibility: Optional[torch.Tensor], R, T, fov, image_size, *, aspect_ratio=None,
                           view_mask=None, damping: float = 1e-6):
    """Damped DLT through the predicted cameras (``_triangulate_joints_dlt``): normalised ``(y, x)`` keypoints (B,V,J,2) ->
    ``(points (B,J,3), valid (B,J) bool)``, ``valid`` where at least two views see the joint.  Per joint the normal equations
    ``(sum a a^T + damping I) p = -sum a a_w`` over the two NDC rows of every seeing view, solved by Cholesky; a joint nobody sees
    comes out as 0.  ``damping`` must be positive: it is what keeps the system definite for a joint seen by fewer than two views.  Gradients go to ``R``, ``T`` and ``fov`` (implicit-function rule); the keypoints carry none."""
    who = "triangulate_joints_dlt"
    kp, vis, vm, R, T, fov, aspect, S, damping = _triangulation_inputs(who, keypoints_2d, visibility, R, T, fov, aspect_ratio, view_mask,
                                                                        image_size, damping)
    device = _on_gpu(kp, R, T, fov, aspect, vis, vm)
    points, valid, _ = _Triangulate.apply(kp.detach().contiguous(), _bytes(vis, device), _bytes(vm, device), R.contiguous(), T.contiguous(),
                                          fov.contiguous(), _c(None if aspect is None else aspect.detach()), S, damping, float("inf"))
    return points, valid.bool()


def triangulation_consistency_loss(keypoints_2d: torch.Tensor, visibility: Optional[torch.Tensor], joints_3d: torch.Tensor, R, T, fov,
                                   image_size, *, aspect_ratio=None, view_mask=None, joint_weights=None, max_norm: float = 50.0,
                                   damping: float = 1e-6) -> torch.Tensor:
    """The triangulation-consistency term (multiview_smil_regressor.py:1050-1110): the keypoints triangulated through the predicted
    cameras against ``joints_3d`` (B,J,3), which is detached, over the joints that are ``valid`` and lie within ``max_norm`` of the
    origin: ``sum w (p - t)^2 / (3 sum w + 1e-8)``, without a trailing eps, and exactly 1e-8 when no joint qualifies.  Gradients go
    to ``R``, ``T`` and ``fov``.  Between its kernels the triangulated points stay float64 whatever the storage type (rounded to
    float32 they would move ``p - t``); the reference's ``isfinite`` fall-back is not reproduced."""
    who = "triangulation_consistency_loss"
    kp, vis, vm, R, T, fov, aspect, S, damping = _triangulation_inputs(who, keypoints_2d, visibility, R, T, fov, aspect_ratio, view_mask,
                                                                        image_size, damping)
    B, J = int(kp.shape[0]), int(kp.shape[2])
    joints_3d = _float_tensor(who, "joints_3d", joints_3d, kp.dtype)
    _shape(who, "joints_3d", joints_3d, (B, J, 3))
    joint_weights = _weights(who, joint_weights, J)
    max_norm = float(max_norm)
    device = _on_gpu(kp, joints_3d, R, T, fov, aspect, vis, vm, joint_weights)
    points, _, sane = _Triangulate.apply(kp.detach().double().contiguous(), _bytes(vis, device), _bytes(vm, device), R.double().contiguous(),
                                         T.double().contiguous(), fov.double().contiguous(),
                                         _c(None if aspect is None else aspect.detach().double()), S, damping, max_norm)
    loss = _SquaredError.apply(points, joints_3d.detach().double().contiguous(), sane, None, _weights_f64(joint_weights, device),
                               _lib.KP_NO_TRAILING_EPS, _lib.KP_POOLED)
    return loss.to(kp.dtype)
