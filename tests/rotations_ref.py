"""The rotation conversions of include/smilfit.h as torch expressions (pytorch3d.transforms 0.7.8's, restated): the reference of the
rotation tests, evaluated in float64 there, with gradients by autograd.  Runs on any device and dtype (tools/rotations_probe.py times
it in float32 as the composition of torch ops the kernels replace)."""
import math

import torch
import torch.nn.functional as F


def rotation_6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)  # a / max(|a|, 1e-12)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def matrix_to_rotation_6d(matrix):
    return matrix[..., :2, :].clone().reshape(matrix.shape[:-2] + (6,))


def _half_sinc(h):
    """sin(h) / (2 h), 1/2 at 0."""
    return 0.5 * torch.sinc(h / math.pi)


def axis_angle_to_quaternion(axis_angle):
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    return torch.cat([torch.cos(angles * 0.5), axis_angle * _half_sinc(angles * 0.5)], dim=-1)


def quaternion_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    t = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - t * (j * j + k * k), t * (i * j - k * r), t * (i * k + j * r),
                     t * (i * j + k * r), 1 - t * (i * i + k * k), t * (j * k - i * r),
                     t * (i * k - j * r), t * (j * k + i * r), 1 - t * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def axis_angle_to_matrix(axis_angle):
    return quaternion_to_matrix(axis_angle_to_quaternion(axis_angle))


def _sqrt_positive_part(x):
    """sqrt(x) for x > 0, else 0, with derivative 0 there."""
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def quaternion_magnitudes(matrix):
    """qa (..., 4): twice the absolute value of each quaternion component a rotation matrix encodes."""
    m = matrix.reshape(matrix.shape[:-2] + (9,))
    m00, m11, m22 = m[..., 0], m[..., 4], m[..., 8]
    return _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1))


def matrix_to_quaternion(matrix):
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(matrix.shape[:-2] + (9,)), dim=-1)
    q_abs = quaternion_magnitudes(matrix)
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    c = q_abs.argmax(dim=-1)  # (the first of equal maxima)
    q = torch.gather(cand, -2, c[..., None, None].expand(c.shape + (1, 4))).squeeze(-2)
    return torch.where(q[..., 0:1] < 0, -q, q)


def quaternion_to_axis_angle(q):
    norms = torch.norm(q[..., 1:], p=2, dim=-1, keepdim=True)
    half_angles = torch.atan2(norms, q[..., :1])
    return q[..., 1:] / _half_sinc(half_angles)


def matrix_to_axis_angle(matrix):
    return quaternion_to_axis_angle(matrix_to_quaternion(matrix))


def axis_angle_to_rotation_6d(axis_angle):
    return matrix_to_rotation_6d(axis_angle_to_matrix(axis_angle))


def rotation_6d_to_axis_angle(d6):
    return matrix_to_axis_angle(rotation_6d_to_matrix(d6))


def rotation_6d_distance(pred6, target6):
    return torch.norm(rotation_6d_to_matrix(pred6) - rotation_6d_to_matrix(target6), p="fro", dim=(-2, -1))


def visibility_weighted_rotation_loss(pred6, target6, visibility):
    """reference smal_fitter/neuralSMIL/smil_image_regressor.py:3157-3186"""
    visible = visibility.bool()
    dist = rotation_6d_distance(pred6, target6)
    num_visible = visible.sum().to(dist.dtype)
    eps = 1e-8
    if num_visible > 0:
        return (dist * visible.to(dist.dtype)).sum() / (num_visible + eps) + eps
    return torch.tensor(eps, dtype=dist.dtype, device=dist.device, requires_grad=True)


def value_and_grads(fn, inputs, weight):
    """``(out, [d (out * weight).sum() / d x for x in inputs])`` of ``fn(*inputs)`` in float64 on the CPU; the inputs' values are taken
    as they are (a float32 tensor is upcast exactly)."""
    xs = [x.detach().cpu().double().requires_grad_(True) for x in inputs]
    out = fn(*xs)
    grads = torch.autograd.grad((out * weight.detach().cpu().double()).sum(), xs)
    return out.detach(), [g.detach() for g in grads]
