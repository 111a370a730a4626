"""Seeded inputs for the keypoint-loss tests (float64 CPU tensors; the tests cast and move them).

The regular set: B samples, V cameras on a ring of radius 3 around the origin looking at it (neighbouring cameras 2 pi / max(V, 3)
apart, jittered by up to 0.2 rad and lifted by up to 0.3 out of the plane), fov in [40, 60] degrees, aspect in [0.8, 1.25], J
joints in the ball of radius ``radius`` (1 by default, so the view-space depth is >= 2; the projection tests use 2: depth >= 1 and
many coordinates clamped).  Targets are the clamped projections plus N(0, 0.02) noise; OUTSIDE_SHARE of the (sample, view, joint)
triples get a target coordinate outside [0,1], INVISIBLE_SHARE are invisible.  A joint whose unclamped projection comes within
1e-6 of 0 or 1 in any view is drawn again, so the branch of the clamp is not a matter of rounding."""
import math

import torch

import keypoint_losses_ref as ref

S = 256
OUTSIDE_SHARE = 0.1
INVISIBLE_SHARE = 0.2
RING_RADIUS = 3.0


def _ball(gen, n, radius):
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    return d * radius * torch.rand(n, 1, generator=gen, dtype=torch.float64).pow(1.0 / 3.0)


def look_at_origin(C):
    """(R, T) of cameras at C (...,3) looking at the origin, up = +y, in the row-vector convention v = X R + T."""
    z = -C / C.norm(dim=-1, keepdim=True)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=C.dtype).expand_as(C)
    x = torch.cross(up, z, dim=-1)
    x = x / x.norm(dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    R = torch.stack([x, y, z], dim=-1)  # the columns are the camera's axes
    T = -(C.unsqueeze(-2) @ R).squeeze(-2)
    return R, T


def regular(B, V, J, seed=0, radius=1.0):
    gen = torch.Generator().manual_seed(1000 + seed)
    u = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    angle = u(B, 1) * 2 * math.pi + torch.arange(V, dtype=torch.float64) * (2 * math.pi / max(V, 3)) + (u(B, V) - 0.5) * 0.4
    C = torch.stack([angle.cos(), (u(B, V) - 0.5) * 0.6, angle.sin()], dim=-1)
    C = RING_RADIUS * C / C.norm(dim=-1, keepdim=True)
    R, T = look_at_origin(C)
    fov, aspect = 40.0 + 20.0 * u(B, V), 0.8 + 0.45 * u(B, V)
    joints = _ball(gen, B * J, radius).reshape(B, J, 3)
    for _ in range(20):
        yx, _depth = ref.project_unclamped(joints, R, T, fov, S, aspect)
        near = (((yx - 0.0).abs() < 1e-6) | ((yx - 1.0).abs() < 1e-6)).any(-1).any(1)  # (B,J)
        if not bool(near.any()):
            break
        joints[near] = _ball(gen, int(near.sum()), radius)
    proj = ref.project_joints_to_views(joints, R, T, fov, S, aspect)
    target = proj + 0.02 * torch.randn(B, V, J, 2, generator=gen, dtype=torch.float64)
    outside = u(B, V, J) < OUTSIDE_SHARE
    far = torch.where(u(B, V, J) < 0.5, -0.05 - 0.45 * u(B, V, J), 1.05 + 0.45 * u(B, V, J))
    which = (u(B, V, J) < 0.5).long().unsqueeze(-1)  # the coordinate that leaves [0,1]
    target = torch.where(outside.unsqueeze(-1) & (torch.arange(2) == which), far.unsqueeze(-1), target)
    inside = ~outside
    target = torch.where(inside.unsqueeze(-1), target.clamp(0.0, 1.0), target)
    visibility = u(B, V, J) >= INVISIBLE_SHARE
    observed = ref.project_unclamped(joints, R, T, fov, S, aspect)[0]  # noise-free observations for the triangulation (not clamped)
    return dict(joints=joints, R=R, T=T, fov=fov, aspect=aspect, proj=proj, observed=observed, target=target, visibility=visibility, outside=outside, S=S)


def check_regular(c, min_depth):
    """The stated properties of a regular set (its sizes permitting)."""
    yx, depth = ref.project_unclamped(c["joints"], c["R"], c["T"], c["fov"], c["S"], c["aspect"])
    if depth.numel():
        assert float(depth.min()) >= min_depth, float(depth.min())
        assert not bool((((yx - 0.0).abs() < 1e-6) | ((yx - 1.0).abs() < 1e-6)).any())
        t = c["target"]
        out = ~((t >= 0) & (t <= 1)).all(-1)
        assert torch.equal(out, c["outside"])


def joint_weights(J, seed=0):
    gen = torch.Generator().manual_seed(2000 + seed)
    return 0.25 + 1.75 * torch.rand(J, generator=gen, dtype=torch.float64)


def upstream(shape, seed=0):
    """Weights of the scalar a test differentiates: sum(out * upstream), in [-1, 1] away from 0."""
    gen = torch.Generator().manual_seed(3000 + seed)
    w = 0.25 + 0.75 * torch.rand(tuple(shape), generator=gen, dtype=torch.float64)
    return w * torch.where(torch.rand(tuple(shape), generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)


def points_3d(N, J, seed=0):
    """3-D prediction / target pairs (N,J,3): targets in the unit ball, predictions 0.05 noise away, visibility at INVISIBLE_SHARE."""
    gen = torch.Generator().manual_seed(4000 + seed)
    target = _ball(gen, N * J, 1.0).reshape(N, J, 3)
    pred = target + 0.05 * torch.randn(N, J, 3, generator=gen, dtype=torch.float64)
    visibility = torch.rand(N, J, generator=gen, dtype=torch.float64) >= INVISIBLE_SHARE
    return pred, target, visibility
