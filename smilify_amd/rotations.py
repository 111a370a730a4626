"""Rotation conversions on the GPU, with pytorch3d.transforms' names and signatures: the step between a regressor's 6-D output and
``SMAL.__call__`` (reference smal_fitter/neuralSMIL/smil_image_regressor.py:26-96, :2597-2669) and its rotation losses (:3117-3266).

Every conversion is a ``torch.autograd.Function`` over one forward and one analytic backward HIP kernel (csrc/rotations.hip; the
formulas are stated at include/smilfit.h).  Tensors are float32 or float64 on the GPU with any leading shape; the arithmetic is
float64 either way.  First-order gradients only.  There is no CPU path: a CPU tensor raises.

A 6-D caller does not need the log map the reference pays for: ``SMAL`` takes ``(B,J,3,3)`` matrices, so
``rotation_6d_to_matrix(d6)`` feeds it directly."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import engine


def _rows(name: str, x: torch.Tensor, tail) -> torch.Tensor:
    """``x`` (..., *tail) as a contiguous (n, prod(tail)) tensor the kernels read; dtype and device are checked here."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype not in engine.ROT_DTYPES:
        raise TypeError(f"{name}: only float32 and float64 are supported, got {x.dtype}")
    engine.require_gpu(x.device)
    width = 1
    for t in tail:
        width *= t
    return x.contiguous().reshape(-1, width)


class _Convert(torch.autograd.Function):
    """out = forward_entry(x); d x = backward_entry(x, d out).  Nothing is saved but the input."""

    @staticmethod
    def forward(ctx, x, fwd, bwd, width):
        ctx.save_for_backward(x)
        ctx.bwd = bwd
        return engine.rot_forward(fwd, x, width)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return engine.rot_backward(ctx.bwd, x, grad.contiguous()), None, None, None


class _Rot6dToAxisAngle(torch.autograd.Function):
    """The fused forward; the backward rebuilds the matrix and runs the two backward kernels.  The matrix and its gradient pass
    through memory there, and they do so as float64 whatever the storage type: rounded to float32 between the kernels they would
    move the point the log map is differentiated at, and the gradient would no longer be a rounding of the float64 one."""

    @staticmethod
    def forward(ctx, d6):
        ctx.save_for_backward(d6)
        return engine.rot_forward("smil_rot6d_to_axis_angle", d6, 3)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (d6,) = ctx.saved_tensors
        d64 = d6.double()
        R = engine.rot_forward("smil_rot6d_to_matrix", d64, 9)
        dR = engine.rot_backward("smil_matrix_to_axis_angle_backward", R, grad.double().contiguous())
        return engine.rot_backward("smil_rot6d_to_matrix_backward", d64, dR).to(d6.dtype)


class _Rot6dDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p6, t6):
        ctx.save_for_backward(p6, t6)
        return engine.rot6d_distance(p6, t6)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        p6, t6 = ctx.saved_tensors
        return engine.rot6d_distance_backward(p6, t6, grad.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def rotation_6d_to_matrix(d6: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> (..., 3, 3): Gram-Schmidt of the two halves, the results are the ROWS of the matrix (Zhou et al. 2019)."""
    if not isinstance(d6, torch.Tensor) or d6.dim() < 1 or d6.shape[-1] != 6:
        raise ValueError(f"Invalid input 6-D rotation shape {tuple(getattr(d6, 'shape', ()))}: the last dimension must be 6.")
    out = _Convert.apply(_rows("rotation_6d_to_matrix", d6, (6,)), "smil_rot6d_to_matrix", "smil_rot6d_to_matrix_backward", 9)
    return out.reshape(d6.shape[:-1] + (3, 3))


def matrix_to_rotation_6d(matrix: torch.Tensor) -> torch.Tensor:
    """(..., 3, 3) -> (..., 6): the first two rows (a slice and a copy; no kernel)."""
    if not isinstance(matrix, torch.Tensor) or matrix.dim() < 2 or tuple(matrix.shape[-2:]) != (3, 3):
        raise ValueError(f"Invalid rotation matrix shape {getattr(matrix, 'shape', None)}.")  # (pytorch3d's wording)
    return matrix[..., :2, :].clone().reshape(matrix.shape[:-2] + (6,))


def axis_angle_to_matrix(axis_angle: torch.Tensor) -> torch.Tensor:
    """(..., 3) -> (..., 3, 3)."""
    if not isinstance(axis_angle, torch.Tensor) or axis_angle.dim() < 1 or axis_angle.shape[-1] != 3:
        raise ValueError(f"Invalid input axis angles shape {tuple(getattr(axis_angle, 'shape', ()))}: the last dimension must be 3.")
    out = _Convert.apply(_rows("axis_angle_to_matrix", axis_angle, (3,)), "smil_axis_angle_to_matrix", "smil_axis_angle_to_matrix_backward", 9)
    return out.reshape(axis_angle.shape[:-1] + (3, 3))


def matrix_to_axis_angle(matrix: torch.Tensor) -> torch.Tensor:
    """(..., 3, 3) -> (..., 3), angle in [0, pi].  Defined for any 3 x 3 input; the axis sign is discontinuous at half turns."""
    if not isinstance(matrix, torch.Tensor) or matrix.dim() < 2 or tuple(matrix.shape[-2:]) != (3, 3):
        raise ValueError(f"Invalid rotation matrix shape {getattr(matrix, 'shape', None)}.")  # (pytorch3d's wording)
    out = _Convert.apply(_rows("matrix_to_axis_angle", matrix, (3, 3)), "smil_matrix_to_axis_angle", "smil_matrix_to_axis_angle_backward", 3)
    return out.reshape(matrix.shape[:-2] + (3,))


def axis_angle_to_rotation_6d(axis_angle: torch.Tensor) -> torch.Tensor:
    """(..., 3) -> (..., 6) (reference smil_image_regressor.py:74-84)."""
    return matrix_to_rotation_6d(axis_angle_to_matrix(axis_angle))


def rotation_6d_to_axis_angle(rotation_6d: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> (..., 3) in one kernel, no matrix in memory (reference smil_image_regressor.py:87-96)."""
    if not isinstance(rotation_6d, torch.Tensor) or rotation_6d.dim() < 1 or rotation_6d.shape[-1] != 6:
        raise ValueError(f"Invalid input 6-D rotation shape {tuple(getattr(rotation_6d, 'shape', ()))}: the last dimension must be 6.")
    out = _Rot6dToAxisAngle.apply(_rows("rotation_6d_to_axis_angle", rotation_6d, (6,)))
    return out.reshape(rotation_6d.shape[:-1] + (3,))


def rotation_6d_distance(pred6: torch.Tensor, target6: torch.Tensor) -> torch.Tensor:
    """(..., 6), (..., 6) -> (...): the Frobenius norm of ``R(pred) - R(target)``.  The gradient goes to either or both inputs and is 0
    where the distance is 0."""
    for name, t in (("pred6", pred6), ("target6", target6)):
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[-1] != 6:
            raise ValueError(f"rotation_6d_distance: {name} must be (..., 6), got {tuple(getattr(t, 'shape', ()))}")
    if pred6.shape != target6.shape:
        raise ValueError(f"rotation_6d_distance: shapes differ, {tuple(pred6.shape)} and {tuple(target6.shape)}")
    p, t = _rows("rotation_6d_distance", pred6, (6,)), _rows("rotation_6d_distance", target6, (6,))
    if p.dtype != t.dtype or p.device != t.device:
        raise TypeError(f"rotation_6d_distance: dtype / device differ, {p.dtype} on {p.device} and {t.dtype} on {t.device}")
    return _Rot6dDistance.apply(p, t).reshape(pred6.shape[:-1])


def visibility_weighted_rotation_loss(pred6: torch.Tensor, target6: torch.Tensor, visibility: torch.Tensor) -> torch.Tensor:
    """The reference's visibility-aware 6-D joint rotation loss (smil_image_regressor.py:3157-3186): ``sum(dist * vis) / (vis.sum() +
    1e-8) + 1e-8`` over the joints whose ``visibility`` (...) is non-zero, and the constant ``1e-8`` (a fresh leaf, as there: no
    gradient reaches the inputs) when none is.  The distances are the kernel's, the reduction is torch's."""
    dist = rotation_6d_distance(pred6, target6)
    visible = torch.as_tensor(visibility, device=dist.device).bool()
    if visible.shape != dist.shape:
        raise ValueError(f"visibility_weighted_rotation_loss: visibility must be {tuple(dist.shape)}, got {tuple(visible.shape)}")
    eps = 1e-8
    num_visible = visible.sum().to(dist.dtype)
    if num_visible > 0:
        return (dist * visible.to(dist.dtype)).sum() / (num_visible + eps) + eps
    return torch.tensor(eps, dtype=dist.dtype, device=dist.device, requires_grad=True)
