"""PointNet++ set abstraction on the HIP kernels: the drop-in for the reference's ``fitter_3d/pointcloud2smil/pointnet2_utils.py``.

Same public names, signatures, tensor shapes and sub-module names (``mlp_convs``, ``mlp_bns``, ``conv_blocks``, ``bn_blocks``: a
``state_dict`` written by the reference loads unchanged).  Farthest point sampling, the ball query and the grouping run in
``csrc/pointnet2.hip``; Conv2d / Conv1d, BatchNorm, ReLU and the max over the neighbours stay torch.  Deviations from the reference
(DESIGN.md section 4.5):

* ties in the farthest-point argmax go to the smallest index;
* the ball query measures ``(dx dx + dy dy) + dz dz`` instead of ``|a|^2 + |b|^2 - 2 a.b``;
* an index outside ``[0, N)`` (the reference's row of N for a query without a hit) groups to a zero row without a gradient instead of
  raising ``IndexError``;
* the coordinates carry no gradient: a call with ``xyz.requires_grad`` raises;
* a cloud holds at most ``SMIL_FPS_MAX_N`` points in ``farthest_point_sample``;
* the start indices come from torch's default CPU generator, or from the ``start_idx=`` keyword.

There is no CPU path: every tensor lives on the GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine

__all__ = ["pc_normalize", "square_distance", "index_points", "farthest_point_sample", "query_ball_point", "sample_and_group",
           "sample_and_group_all", "PointNetSetAbstraction", "PointNetSetAbstractionMsg", "PointNetFeaturePropagation"]


def pc_normalize(pc):
    """A numpy cloud (N, 3) moved to its centroid and scaled into the unit ball."""
    pc = pc - np.mean(pc, axis=0)
    return pc / np.max(np.sqrt(np.sum(pc ** 2, axis=1)))


def square_distance(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """(B, N, M) squared distances of src (B, N, C) and dst (B, M, C) in the expanded form |a|^2 + |b|^2 - 2 a.b (plain torch: nothing
    on the kernels' path uses it)."""
    return -2.0 * torch.matmul(src, dst.transpose(1, 2)) + (src ** 2).sum(-1)[:, :, None] + (dst ** 2).sum(-1)[:, None, :]


def _gpu_f32(t: torch.Tensor) -> torch.Tensor:
    engine.require_gpu(t.device)
    return t.to(torch.float32).contiguous()


def _no_coordinate_gradient(what: str, *tensors) -> None:
    if any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: the coordinates carry no gradient on the HIP path; detach them first")


class _GroupFn(torch.autograd.Function):
    """engine.group_points with the gradient to the features."""

    @staticmethod
    def forward(ctx, features, xyz, centres, idx, xyz_last):
        ctx.save_for_backward(idx)
        ctx.layout = (None if features is None else tuple(features.shape[1:]), xyz is not None, bool(xyz_last))
        return engine.group_points(xyz, centres, features, idx, xyz_last)

    @staticmethod
    def backward(ctx, d_out):
        (idx,) = ctx.saved_tensors
        shape, has_xyz, xyz_last = ctx.layout
        d = None
        if shape is not None and ctx.needs_input_grad[0]:
            d = engine.group_points_backward(d_out.contiguous(), idx, shape[0], shape[1], has_xyz, xyz_last)
        return d, None, None, None, None


def _group(xyz, centres, features, idx, xyz_last=False) -> torch.Tensor:
    """(B, C, K, S) contiguous, the layout Conv2d reads; idx (B, S, K) of any integer type."""
    _no_coordinate_gradient("grouping", xyz, centres)
    return _GroupFn.apply(None if features is None else _gpu_f32(features), None if xyz is None else _gpu_f32(xyz),
                          None if centres is None else _gpu_f32(centres), idx.to(torch.int32).contiguous(), xyz_last)


def index_points(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """points (B, N, C) at idx (B, S) or (B, S, K): (B, S, C) or (B, S, K, C), a view of the kernel's channel-major result.  An index
    outside [0, N) gives a zero row."""
    if idx.dim() not in (2, 3):
        raise ValueError("index_points: idx must be (B, S) or (B, S, K)")
    out = _group(None, None, points, idx if idx.dim() == 3 else idx[:, :, None]).permute(0, 3, 2, 1)
    return out if idx.dim() == 3 else out[:, :, 0]


def farthest_point_sample(xyz: torch.Tensor, npoint: int, start_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, npoint) int64 indices of xyz (B, N, 3), column 0 the start index.  ``start_idx`` (B): the start of every cloud (an
    extension); otherwise ``torch.randint(0, N, (B,))`` from the default CPU generator, so ``torch.manual_seed`` governs it."""
    if not (isinstance(xyz, torch.Tensor) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("farthest_point_sample: xyz must be (B, N, 3)")
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    if start_idx is None:
        start_idx = torch.randint(0, N, (B,), dtype=torch.long)
    elif tuple(start_idx.shape) != (B,) or bool(((start_idx < 0) | (start_idx >= N)).any()):
        raise ValueError(f"farthest_point_sample: start_idx must hold B={B} indices in [0, {N})")
    x = _gpu_f32(xyz.detach())
    return engine.fps(x, int(npoint), start_idx.to(device=x.device, dtype=torch.int32)).long()


def _ball_query(radii: Sequence[float], nsamples: Sequence[int], xyz: torch.Tensor, new_xyz: torch.Tensor):
    return engine.ball_query(_gpu_f32(xyz.detach()), _gpu_f32(new_xyz.detach()), radii, nsamples)


def query_ball_point(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
    """(B, S, min(nsample, N)) int64: per query of new_xyz (B, S, 3) the first indices of xyz (B, N, 3) within the radius, ascending,
    padded with the first; a query without a hit holds N."""
    return _ball_query([radius], [nsample], xyz, new_xyz)[0].long()


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False):
    """new_xyz (B, npoint, 3) and new_points (B, npoint, nsample, 3 + D) = [grouped xyz - centre, grouped points]; with ``returnfps``
    also grouped_xyz (B, npoint, nsample, 3) and fps_idx (B, npoint)."""
    _no_coordinate_gradient("sample_and_group", xyz)
    fps_idx = farthest_point_sample(xyz, npoint)
    new_xyz = index_points(xyz, fps_idx).contiguous()
    idx = _ball_query([radius], [nsample], xyz, new_xyz)[0]
    new_points = _group(xyz, new_xyz, points, idx).permute(0, 3, 2, 1)
    if returnfps:
        return new_xyz, new_points, index_points(xyz, idx), fps_idx
    return new_xyz, new_points


def sample_and_group_all(xyz, points):
    """The whole cloud as one group: new_xyz (B, 1, 3) zeros, new_points (B, 1, N, 3 + D)."""
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device, dtype=xyz.dtype)
    grouped = xyz.reshape(B, 1, N, C)
    return new_xyz, grouped if points is None else torch.cat([grouped, points.reshape(B, 1, N, -1)], dim=-1)


def _mlp(x, convs, bns):
    for conv, bn in zip(convs, bns):
        x = F.relu(bn(conv(x)))
    return x


def _conv_stack(conv, bn, channels, widths):
    convs, bns = nn.ModuleList(), nn.ModuleList()
    for width in widths:
        convs.append(conv(channels, width, 1))
        bns.append(bn(width))
        channels = width
    return convs, bns


class PointNetSetAbstraction(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs, self.mlp_bns = _conv_stack(nn.Conv2d, nn.BatchNorm2d, in_channel, mlp)

    def forward(self, xyz, points):
        """xyz (B, 3, N), points (B, D, N) or None -> new_xyz (B, 3, S), new_points (B, D', S)."""
        xyz = xyz.transpose(1, 2)
        points = None if points is None else points.transpose(1, 2)
        if self.group_all:
            new_xyz, new_points = sample_and_group_all(xyz, points)
        else:
            new_xyz, new_points = sample_and_group(self.npoint, self.radius, self.nsample, xyz, points)
        grouped = new_points.permute(0, 3, 2, 1)  # (B, C, K, S): contiguous again when it came from the kernel
        return new_xyz.transpose(1, 2), _mlp(grouped, self.mlp_convs, self.mlp_bns).max(2)[0]


class PointNetSetAbstractionMsg(nn.Module):
    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for widths in mlp_list:
            convs, bns = _conv_stack(nn.Conv2d, nn.BatchNorm2d, in_channel + 3, widths)
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points):
        """xyz (B, 3, N), points (B, D, N) or None -> new_xyz (B, 3, S), the scales' features concatenated (B, D', S)."""
        _no_coordinate_gradient("PointNetSetAbstractionMsg", xyz)
        xyz = xyz.transpose(1, 2).contiguous()
        points = None if points is None else points.transpose(1, 2)
        new_xyz = index_points(xyz, farthest_point_sample(xyz, self.npoint)).contiguous()
        scales = []
        radii, nsamples = list(self.radius_list), list(self.nsample_list)
        for r0 in range(0, len(radii), engine._lib.BALL_MAX_RADII):  # one pass over the candidates per four radii
            for i, idx in enumerate(_ball_query(radii[r0:r0 + 4], nsamples[r0:r0 + 4], xyz, new_xyz), start=r0):
                grouped = _group(xyz, new_xyz, points, idx, xyz_last=True)
                scales.append(_mlp(grouped, self.conv_blocks[i], self.bn_blocks[i]).max(2)[0])
        return new_xyz.transpose(1, 2), torch.cat(scales, dim=1)


class PointNetFeaturePropagation(nn.Module):
    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns = _conv_stack(nn.Conv1d, nn.BatchNorm1d, in_channel, mlp)

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 (B, 3, N), xyz2 (B, 3, S), points1 (B, D1, N) or None, points2 (B, D2, S) -> (B, D', N): points2 interpolated to xyz1
        from the three nearest of xyz2 with inverse squared-distance weights, then the MLP."""
        from .fit3d import knn_points

        xyz1, xyz2, points2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2), points2.transpose(1, 2)
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:
            interpolated = points2.repeat(1, N, 1)
        else:
            _no_coordinate_gradient("PointNetFeaturePropagation", xyz1, xyz2)
            nn3 = knn_points(_gpu_f32(xyz1), _gpu_f32(xyz2), K=min(3, S))
            weight = 1.0 / (nn3.dists + 1e-8)
            weight = weight / weight.sum(dim=2, keepdim=True)
            interpolated = (index_points(points2, nn3.idx) * weight[..., None]).sum(dim=2)
        new_points = interpolated if points1 is None else torch.cat([points1.transpose(1, 2), interpolated], dim=-1)
        return _mlp(new_points.transpose(1, 2), self.mlp_convs, self.mlp_bns)
