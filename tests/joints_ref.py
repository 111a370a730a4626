"""TEST INFRASTRUCTURE ONLY: the 3-D keypoint term of ``smilify_amd/csrc/joints.hip`` restated in float64 torch (autograd gives its
gradients), and the composition ``oracle joints -> term``.  The joints come from ``oracle/lbs_ref.py`` (dense LBS over every vertex) on
``lbs_ref64.dense_model`` tables; the window sizes from ``fit_ref.window_sizes``.  Holds no kernels and touches no GPU.

    term = w_k3d sum_w 1/(3 Jc b_w) sum_{n in w} sum_c vis[n,c] wj[c] rho(|joints[n, canon[c]] - target[n,c]|^2)

rho(s) = s (robust_scale == 0) or 2 sigma^2 (sqrt(1 + s / sigma^2) - 1); a target row that is exactly (0,0,0) or holds a non-finite
entry is invisible.
"""
import torch

import fit_ref
import lbs_ref64
from oracle import lbs_ref

F64 = torch.float64


def visible(target, visibility=None):
    """(N,Jc) bool: the entries the term sees."""
    t = torch.as_tensor(target)
    seen = torch.isfinite(t).all(-1) & (t != 0).any(-1)
    if visibility is not None:
        seen = seen & (torch.as_tensor(visibility) != 0)
    return seen


def kp3d_term(joints, target, visibility=None, joint_weights=None, canon=None, w_k3d=1.0, robust_scale=0.0, window=0, frame0=0,
              N_total=None):
    """The term as a float64 scalar, differentiable in ``joints`` (N,J,3)."""
    N, Jc = target.shape[0], target.shape[1]
    seen = visible(target, visibility)
    tgt = torch.where(seen[..., None], torch.as_tensor(target).to(F64), torch.zeros((), dtype=F64))
    sel = joints[:, :Jc] if canon is None else joints[:, torch.as_tensor(canon, dtype=torch.long)]
    s = ((sel - tgt) ** 2).sum(-1)
    if robust_scale > 0:
        s2 = float(robust_scale) ** 2
        rho = 2.0 * s2 * (torch.sqrt(1.0 + s / s2) - 1.0)
    else:
        rho = s
    wj = torch.ones(Jc, dtype=F64) if joint_weights is None else torch.as_tensor(joint_weights).to(F64)
    bw = fit_ref.window_sizes(N, window, frame0, N_total)[:, None]
    return float(w_k3d) * (seen.to(F64) * wj[None] * rho / (3.0 * Jc * bw)).sum()


def oracle_joints(t, betas, pose, trans, log_beta_scales, betas_trans, mask, propagate_scaling=False, allow_limb_scaling=True):
    """Posed joints (N,J,3) of the fitter convention in float64 from the dense oracle: betas (nB,), pose (N,J,3) unmasked, mask (J,3),
    trans (N,3), the scale tables (J,3) or None.  Differentiable in every float64 leaf passed in."""
    N = pose.shape[0]
    m = lbs_ref64.dense_model(t, F64)
    ex = lambda x: None if x is None else x[None].expand(N, *x.shape)  # noqa: E731
    o = lbs_ref.smal_forward(m, betas[None].expand(N, -1), pose * torch.as_tensor(mask).to(F64), trans=None, betas_logscale=ex(log_beta_scales),
                             betas_trans=ex(betas_trans), propagate_scaling=propagate_scaling, allow_limb_scaling=allow_limb_scaling)
    return o["joints"] + trans[:, None]


def fit_eval(t, params, mask, target, visibility, joint_weights, canon, w_k3d, robust_scale, window):
    """``oracle joints -> term`` on float32 parameters: (term, joints, gradients on betas, pose (with respect to the MASKED pose), trans,
    log_beta_scales, betas_trans), all float64.  ``params``: dict of float32 tensors with those names."""
    leaves = {k: torch.as_tensor(v).detach().to(F64).clone().requires_grad_() for k, v in params.items()}
    masked = leaves["pose"] * torch.as_tensor(mask).to(F64)
    masked.retain_grad()
    joints = oracle_joints(t, leaves["betas"], masked, leaves["trans"], leaves.get("log_beta_scales"), leaves.get("betas_trans"),
                           torch.ones_like(torch.as_tensor(mask)))
    term = kp3d_term(joints, target, visibility, joint_weights, canon, w_k3d, robust_scale, window)
    if term.requires_grad:
        term.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in leaves.items() if k != "pose"}
    grads["pose"] = torch.zeros_like(masked) if masked.grad is None else masked.grad.detach()
    return term.detach(), joints.detach(), grads
