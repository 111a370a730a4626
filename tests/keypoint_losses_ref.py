"""A float64 torch restatement of smilify_amd.keypoint_losses, written from the formulas at include/smilfit.h with plain tensor
operations and ``torch.linalg.solve``; autograd supplies the gradients.  Every function upcasts its inputs to float64 (exact for
float32) and runs where they live (the tests call it on the CPU)."""
import math

import torch

EPS = 1e-8


def _on(x, like):
    return None if x is None else torch.as_tensor(x).to(like.device)


def _true(x, like_shape, device):
    """non-zero -> True; None -> all True"""
    return torch.ones(like_shape, dtype=torch.bool, device=device) if x is None else (x != 0)


def _reduce(pred, target, valid, selected, weights, D, reduction, trailing_eps=True):
    """pred, target (*lead, J, D) float64, valid (*lead, J) bool, selected (*lead) bool."""
    J = pred.shape[-2]
    w = torch.ones(J, dtype=torch.float64, device=pred.device) if weights is None else _on(weights, pred).double()
    vw = valid.double() * w
    err = torch.where(valid.unsqueeze(-1), pred - target, torch.zeros_like(pred)).pow(2).sum(-1)
    num, count = (vw * err).sum(-1), vw.sum(-1)
    if reduction == "pooled":
        if not trailing_eps:
            return num.sum() / (D * count.sum() + EPS) if bool(valid.any()) else num.sum() * 0.0 + EPS
        return num.sum() / (D * count.sum() + EPS) + EPS
    if reduction == "valid_samples":
        included = valid.any(-1)
    elif reduction == "samples":
        included = selected
    else:
        raise ValueError(reduction)
    n = int(included.sum())
    if n == 0:
        return num.sum() * 0.0 + EPS
    return (num / (D * count + EPS) * included.double()).sum() / n + EPS


def keypoint_loss_2d(rendered, target, visibility, joint_weights=None, mask=None, reduction="pooled"):
    r, t = rendered.double(), target.detach().double()
    r = torch.where(torch.isfinite(r), r, torch.zeros_like(r))  # a non-finite coordinate counts as 0, without a gradient
    selected = _true(_on(mask, r), r.shape[:-2], r.device)
    valid = ((t >= 0.0) & (t <= 1.0)).all(-1) & _true(_on(visibility, r), r.shape[:-1], r.device) & selected.unsqueeze(-1)
    return _reduce(r, t, valid, selected, joint_weights, 2, reduction)


def keypoint_loss_3d(joints, target, visibility, joint_weights=None, mask=None, reduction="valid_samples"):
    p, t = joints.double(), target.detach().double()
    selected = _true(_on(mask, p), p.shape[:-2], p.device)
    valid = torch.isfinite(p).all(-1) & torch.isfinite(t).all(-1) & (t.abs().sum(-1) > 0.0)
    valid = valid & _true(_on(visibility, p), p.shape[:-1], p.device) & selected.unsqueeze(-1)
    return _reduce(p, t, valid, selected, joint_weights, 3, reduction)


def focal(fov, aspect_ratio=None):
    """(k00, k11) of FoV cameras, fov in degrees"""
    k11 = 1.0 / torch.tan(fov.double() * (math.pi / 360.0))
    return (k11 if aspect_ratio is None else k11 / aspect_ratio.double()), k11


def project_unclamped(joints_3d, R, T, fov, image_size, aspect_ratio=None):
    """(B,V,J,2): (y, x) / (S + 1e-8) before the clamp, and the view-space depth (B,V,J)"""
    X, R, T, S = joints_3d.double(), R.double(), T.double(), float(image_size)
    v = torch.einsum("bjk,bvkc->bvjc", X, R) + T.unsqueeze(2)
    k00, k11 = focal(fov, aspect_ratio)
    x_ndc = k00.unsqueeze(-1) * v[..., 0] / v[..., 2]
    y_ndc = k11.unsqueeze(-1) * v[..., 1] / v[..., 2]
    yx = torch.stack([S / 2 - S / 2 * y_ndc, S / 2 - S / 2 * x_ndc], dim=-1)
    return yx / (S + 1e-8), v[..., 2]


def project_joints_to_views(joints_3d, R, T, fov, image_size, aspect_ratio=None):
    return project_unclamped(joints_3d, R, T, fov, image_size, aspect_ratio)[0].clamp(0.0, 1.0)


def multiview_keypoint_loss(joints_3d, R, T, fov, target, visibility, image_size, aspect_ratio=None, view_mask=None, joint_weights=None):
    return keypoint_loss_2d(project_joints_to_views(joints_3d, R, T, fov, image_size, aspect_ratio), target, visibility, joint_weights,
                            view_mask, "pooled")


def dlt_system(keypoints_2d, visibility, R, T, fov, image_size, aspect_ratio=None, view_mask=None, damping=1e-6):
    """(M (B,J,3,3) with the damping, c (B,J,3), seen (B,V,J) bool)"""
    kp, R, T, S = keypoints_2d.detach().double(), R.double(), T.double(), float(image_size)
    B, V, J, _ = kp.shape
    k00, k11 = focal(fov, aspect_ratio)
    u = 1.0 - (kp[..., 1] * S) / (S / 2)
    v = 1.0 - (kp[..., 0] * S) / (S / 2)
    col = [torch.cat([R[..., :, i], T[..., i:i + 1]], dim=-1).unsqueeze(2) for i in range(3)]  # (B,V,1,4) each
    row1 = u.unsqueeze(-1) * col[2] - k00[..., None, None] * col[0]
    row2 = v.unsqueeze(-1) * col[2] - k11[..., None, None] * col[1]
    seen = _true(_on(visibility, kp), (B, V, J), kp.device) & _true(_on(view_mask, kp), (B, V), kp.device).unsqueeze(-1)
    A = torch.stack([row1, row2], dim=3)  # (B,V,J,2,4)
    A = torch.where(seen[..., None, None], A, torch.zeros_like(A)).permute(0, 2, 1, 3, 4).reshape(B, J, 2 * V, 4)
    A_xyz, a_w = A[..., :3], A[..., 3]
    M = A_xyz.transpose(-1, -2) @ A_xyz + damping * torch.eye(3, dtype=torch.float64, device=kp.device)
    c = -(A_xyz.transpose(-1, -2) @ a_w.unsqueeze(-1)).squeeze(-1)
    return M, c, seen


def triangulate_joints_dlt(keypoints_2d, visibility, R, T, fov, image_size, aspect_ratio=None, view_mask=None, damping=1e-6):
    M, c, seen = dlt_system(keypoints_2d, visibility, R, T, fov, image_size, aspect_ratio, view_mask, damping)
    return torch.linalg.solve(M, c), seen.sum(dim=1) >= 2


def triangulation_consistency_loss(keypoints_2d, visibility, joints_3d, R, T, fov, image_size, aspect_ratio=None, view_mask=None,
                                   joint_weights=None, max_norm=50.0, damping=1e-6):
    p, valid = triangulate_joints_dlt(keypoints_2d, visibility, R, T, fov, image_size, aspect_ratio, view_mask, damping)
    sane = valid & (p.detach().norm(dim=-1) < max_norm)
    selected = torch.ones(p.shape[:-2], dtype=torch.bool, device=p.device)
    return _reduce(p, joints_3d.detach().double(), sane, selected, joint_weights, 3, "pooled", trailing_eps=False)


def value_and_grads(fn, inputs, wrt, upstream=None):
    """``fn(*inputs)`` with the tensors named by the indices ``wrt`` as float64 CPU leaves; returns (value, [gradient per index])
    of ``(value * upstream).sum()``; an input the value does not depend on gets zeros."""
    args = [a.detach().cpu().double() if isinstance(a, torch.Tensor) and a.is_floating_point() else
            (a.detach().cpu() if isinstance(a, torch.Tensor) else a) for a in inputs]
    for i in wrt:
        args[i].requires_grad_(True)
    out = fn(*args)
    value = out[0] if isinstance(out, tuple) else out
    total = value.sum() if upstream is None else (value * upstream.detach().cpu().double()).sum()
    grads = torch.autograd.grad(total, [args[i] for i in wrt], allow_unused=True) if total.requires_grad else [None] * len(wrt)
    return out, [torch.zeros_like(args[i]) if g is None else g for i, g in zip(wrt, grads)]
