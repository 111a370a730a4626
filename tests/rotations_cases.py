"""Seeded inputs of the rotation tests (float64 CPU tensors; a float32 test casts them and the reference sees the cast values).

The sets are the ones the tolerances of test_gpu_rotations.py are derived for; ``check_regular`` asserts the stated ranges on the
values a test actually uses."""
import math

import numpy as np
import torch

import rotations_ref as ref

REGULAR_SEED = 20261
QA_GAP = 1e-6  # the two largest quaternion magnitudes of a regular matrix differ by at least this (the candidate is unambiguous)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def regular(n, seed=REGULAR_SEED):
    """n rotations in general position: ``aa`` (n,3) with angles in [1e-3, pi - 1e-2], ``R`` (n,3,3) its matrix, and ``d6`` (n,6) a
    6-D row of the SAME rotation with |a1| and |a2| in [0.1, 10] and the angle between a1 and a2 in [0.1, pi - 0.1]."""
    rng = np.random.default_rng(seed)
    angle = rng.uniform(1e-3, math.pi - 1e-2, n)
    aa = torch.from_numpy(_unit(rng, n) * angle[:, None])
    R = ref.axis_angle_to_matrix(aa)
    s1, s2 = _log_uniform(rng, 0.1, 10.0, n), _log_uniform(rng, 0.1, 10.0, n)
    phi = rng.uniform(0.1, math.pi - 0.1, n)
    r1, r2 = R[:, 0].numpy(), R[:, 1].numpy()
    d6 = np.concatenate([s1[:, None] * r1, s2[:, None] * (np.cos(phi)[:, None] * r1 + np.sin(phi)[:, None] * r2)], axis=1)
    return dict(aa=aa, R=R, d6=torch.from_numpy(d6))


def check_regular(d6=None, R=None, aa=None):
    """Assert, on the values a test feeds the kernels (float64 upcasts of them), that every row lies in the regular set."""
    if d6 is not None:
        d6 = d6.detach().cpu().double()
        a1, a2 = d6[:, :3], d6[:, 3:]
        n1, n2 = a1.norm(dim=1), a2.norm(dim=1)
        assert bool(((n1 >= 0.0999) & (n1 <= 10.001)).all()), "regular set: |a1| outside [0.1, 10]"
        phi = torch.acos(((a1 * a2).sum(1) / (n1 * n2)).clamp(-1, 1))
        assert bool(((phi >= 0.0999) & (phi <= math.pi - 0.0999)).all()), "regular set: angle(a1, a2) outside [0.1, pi - 0.1]"
        R = ref.rotation_6d_to_matrix(d6) if R is None else R
    if aa is not None:
        ang = aa.detach().cpu().double().norm(dim=1)
        assert bool(((ang >= 0.999e-3) & (ang <= math.pi - 0.999e-2)).all()), "regular set: rotation angle outside [1e-3, pi - 1e-2]"
    if R is not None:
        R = R.detach().cpu().double().reshape(-1, 3, 3)
        top = ref.quaternion_magnitudes(R).topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
        assert bool((gap >= QA_GAP).all()), f"regular set: the two largest qa are {float(gap.min()):.3g} apart in some row (< {QA_GAP})"
        sin_ang = 0.5 * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=1).norm(dim=1)
        ang = torch.atan2(sin_ang, 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0))
        assert bool(((ang >= 0.99e-3) & (ang <= math.pi - 0.99e-2)).all()), "regular set: a matrix's angle outside [1e-3, pi - 1e-2]"


def _skew(v):
    x, y, z = v
    return torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=torch.float64)


SMALL_ANGLES = (0.0, 1e-12, 1e-7, 1e-4)


def small_angle():
    """``aa`` (12,3): three axes at each of the angles 0, 1e-12, 1e-7, 1e-4; ``R`` (14,3,3): their matrices, the identity and
    I + 1e-7 skew(axis)."""
    axes = torch.tensor([[1.0, 0.0, 0.0], [0.6, -0.8, 0.0], [1.0, 2.0, -2.0]], dtype=torch.float64)
    axes = axes / axes.norm(dim=1, keepdim=True)
    aa = torch.cat([axes * t for t in SMALL_ANGLES])
    extra = torch.stack([torch.eye(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64) + 1e-7 * _skew(axes[2].tolist())])
    return dict(aa=aa, R=torch.cat([ref.axis_angle_to_matrix(aa), extra]))


def degenerate_6d():
    """The ten degenerate 6-D rows (every product in them is exact, so u = a2 - (b1 . a2) b1 is an exact zero where a2 || a1)."""
    return torch.tensor([
        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],       # zeros: the zero matrix
        [1.0, 0.0, 0.0, 2.0, 0.0, 0.0],       # a2 || a1: b2 = b3 = 0
        [0.0, 3.0, 0.0, 0.0, -5.0, 0.0],      # a2 anti-parallel to a1
        [1e-13, 0.0, 0.0, 0.0, 1.0, 0.0],     # |a1| under the clamp: b1 = (0.1, 0, 0)
        [0.0, 0.0, 1e-13, 1.0, 0.0, 0.0],
        [1.0, 0.0, 0.0, 1.0, 1e-13, 0.0],     # |u| under the clamp: b2 = (0, 0.1, 0)
        [0.0, 0.0, 0.0, 1.0, 2.0, 3.0],       # a1 = 0: b1 = b3 = 0, b2 = a2 / |a2|
        [2.0, 0.0, 0.0, 4.0, 0.0, 0.0],
        [0.0, 0.0, 0.0, 0.0, 2.0, 0.0],
        [1.0, 2.0, 3.0, 0.0, 0.0, 0.0],       # a2 = 0
    ], dtype=torch.float64)


HALF_TURN_ANGLES = (math.pi - 1e-6, math.pi, math.pi + 1e-3, 2.0 * math.pi - 1e-3)


def half_turn():
    """``R`` (12,3,3): three axes at angles around a half turn and just under a full one, where the returned axis sign (or the angle's
    branch) is discontinuous: compare matrices rebuilt from the result."""
    axes = torch.tensor([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [1.0, 2.0, -2.0]], dtype=torch.float64)
    axes = axes / axes.norm(dim=1, keepdim=True)
    return ref.axis_angle_to_matrix(torch.cat([axes * t for t in HALF_TURN_ANGLES]))


def weights(shape, seed):
    """Upstream gradients in [-1, 1] with |w| >= 0.25: every output element takes part in the gradient."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
    return torch.from_numpy(w)


NEAR_DISTANCE = (2e-6, 1e-4)  # what "a distance of ~1e-5" means for the near pairs


def distance_pairs(n, seed=REGULAR_SEED):
    """``(p, t, q, q_near)``: regular 6-D rows p and unrelated regular rows t; rows q and rows 2e-5 away from them in the 6-D space,
    which puts the matrices ~1e-5 apart (``NEAR_DISTANCE`` is asserted by the test).  The near pairs are well conditioned, |a1|, |a2|
    in [0.5, 2] and angle(a1, a2) in [pi/4, 3 pi/4]: the difference of two matrices 1e-5 apart loses five of the sixteen digits, so the
    unit direction of the gradient carries ~1e-16 / 1e-5 = 1e-11 per rounding, and the 1e-10 bound has room for a few of those but not
    for another factor 100 from the Gram-Schmidt step or a ten times smaller distance."""
    p, t = regular(n, seed)["d6"], regular(n, seed + 1)["d6"]
    rng = np.random.default_rng(seed + 2)
    R = ref.axis_angle_to_matrix(torch.from_numpy(_unit(rng, n) * rng.uniform(0.1, 3.0, n)[:, None])).numpy()
    phi = rng.uniform(math.pi / 4, 3 * math.pi / 4, n)
    s1, s2 = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    q = np.concatenate([s1[:, None] * R[:, 0], s2[:, None] * (np.cos(phi)[:, None] * R[:, 0] + np.sin(phi)[:, None] * R[:, 1])], axis=1)
    step = rng.standard_normal(q.shape)
    near = q + 2e-5 * step / np.linalg.norm(step, axis=1, keepdims=True)
    return p, t, torch.from_numpy(q), torch.from_numpy(near)
