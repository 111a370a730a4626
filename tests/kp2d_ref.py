"""TEST INFRASTRUCTURE ONLY: the multi-view 2-D keypoint term of ``smilify_amd/csrc/joints.hip`` (smil_kp2d_fit_eval) restated in torch
from the header comment of ``include/smilfit.h`` (autograd gives its gradients), and the composition ``oracle joints -> 2-D term (+ 3-D
term)``.  The projection is ``pinhole_ref.project_points_screen``, the window sizes ``fit_ref.window_sizes``, the joints
``joints_ref.oracle_joints`` (dense LBS over every vertex).  Holds no kernels and touches no GPU.

    term = w_k2d sum_w 1/(2 Jc Nv b_w) sum_{n in w} sum_v sum_c seen[n,v,c] conf[n,v,c] wj[c] rho(|yx(joints[n,canon[c]]; cam(n,v)) - target[n,v,c]|^2)

Image ``n * Nv + v``; a camera table with k rows (k = 1, Nv or N * Nv) is indexed ``image % k``.  ``cams``: dict with ``R (k,3,3)``, ``T (k,3)``,
``fov (k,)`` degrees and optionally ``aspect (k,)`` and ``principal (k,2)``.
"""
import numpy as np
import torch

import fit_ref
import joints_ref
import lbs_ref64
import pinhole_ref
from oracle import lbs_ref

F64 = torch.float64
ZNEAR = float(np.float32(0.001))  # SMIL_ZNEAR as the kernels hold it


def project(points, cams, S, views):
    """points (N,P,3) -> yx (N,Nv,P,2) in (y,x) pixels and the view depth z (N,Nv,P), in the dtype of ``points``."""
    N, P = points.shape[0], points.shape[1]
    n_img, dt = N * views, points.dtype
    tab = {k: (None if cams.get(k) is None else pinhole_ref.rows(torch.as_tensor(cams[k]).reshape(-1, *s), n_img).to(dt))
           for k, s in (("R", (3, 3)), ("T", (3,)), ("fov", ()), ("aspect", ()), ("principal", (2,)))}
    tab = {k: (None if v is None else v.to(points.device)) for k, v in tab.items()}
    pe = points[:, None].expand(-1, views, -1, -1).reshape(n_img, P, 3)
    if dt == F64:
        ndc = pinhole_ref.project_to_ndc(pe, tab["R"], tab["T"], tab["fov"], tab["aspect"], tab["principal"])
    else:  # (pinhole_ref always computes in float64: the float32 evaluation restates its three lines)
        from oracle import render_ref

        ndc = render_ref.project_to_ndc(pe, tab["R"], tab["T"], tab["fov"], tab["aspect"])
        if tab["principal"] is not None:
            ndc = torch.cat([ndc[..., :2] + tab["principal"][:, None, :], ndc[..., 2:]], dim=-1)
    yx = pinhole_ref.ndc_to_screen(ndc, S)
    return yx.reshape(N, views, P, 2), ndc[..., 2].reshape(N, views, P)


def seen_entries(target, z, visibility=None, confidence=None):
    """(N,Nv,Jc) bool - the seen rule, written once: visibility (if given) non-zero, both target coordinates finite, the confidence (if
    given) finite and > 0, and the view depth of the joint > SMIL_ZNEAR."""
    seen = torch.isfinite(torch.as_tensor(target)).all(-1) & (z.detach().to(F64) > ZNEAR)
    if visibility is not None:
        seen = seen & (torch.as_tensor(visibility) != 0)
    if confidence is not None:
        c = torch.as_tensor(confidence)
        seen = seen & torch.isfinite(c) & (c > 0)
    return seen


def _select(joints, canon, Jc):
    return joints[:, :Jc] if canon is None else joints[:, torch.as_tensor(canon, dtype=torch.long)]


def kp2d_term(joints, cams, S, target, visibility=None, confidence=None, joint_weights=None, canon=None, w_k2d=1.0, robust_scale_px=0.0,
              window=0, frame0=0, N_total=None, with_projection=False):
    """The term as a scalar of the dtype of ``joints`` (N,J,3), differentiable in ``joints``.  ``with_projection``: also the projections of
    the canonical joints ``yx (N,Nv,Jc,2)`` (NaN where the depth rule fails) and ``seen (N,Nv,Jc)``."""
    dt, dev = joints.dtype, joints.device  # (the GPU file evaluates this expression on the device too: fused against unfused)
    on = lambda x: None if x is None else torch.as_tensor(x).to(dev)  # noqa: E731
    target, visibility, confidence, joint_weights = on(target), on(visibility), on(confidence), on(joint_weights)
    N, Nv, Jc = target.shape[0], target.shape[1], target.shape[2]
    yx, z = project(_select(joints, canon, Jc), cams, S, Nv)
    seen = seen_entries(target, z, visibility, confidence)
    zero = torch.zeros((), dtype=dt)
    res = torch.where(seen[..., None], yx - torch.where(torch.isfinite(target), target, torch.zeros(())).to(dt), zero)
    s = (res ** 2).sum(-1)
    if robust_scale_px > 0:
        s2 = float(robust_scale_px) ** 2
        rho = 2.0 * s2 * (torch.sqrt(1.0 + s / s2) - 1.0)
    else:
        rho = s
    wj = torch.ones(Jc, dtype=dt, device=dev) if joint_weights is None else joint_weights.to(dt)
    conf = torch.ones((), dtype=dt) if confidence is None else torch.where(seen, torch.as_tensor(confidence).to(dt), zero)
    bw = fit_ref.window_sizes(N, window, frame0, N_total).to(dev, dt)[:, None, None]
    term = float(w_k2d) * (seen.to(dt) * conf * wj[None, None] * rho / (2.0 * Jc * Nv * bw)).sum()
    if not with_projection:
        return term
    nan = torch.full((), float("nan"), dtype=dt)
    return term, torch.where((z.detach().to(F64) > ZNEAR)[..., None], yx.detach(), nan), seen


def kp3d_term(joints, target, visibility=None, joint_weights=None, canon=None, w_k3d=1.0, robust_scale=0.0, window=0):
    """``joints_ref.kp3d_term``; in float32 when the joints are (that function casts its operands to float64), so that the float32
    evaluation of a problem with both terms measures both."""
    dt = joints.dtype
    if dt == F64:
        return joints_ref.kp3d_term(joints, target, visibility, joint_weights, canon, w_k3d, robust_scale, window)
    N, Jc = target.shape[0], target.shape[1]
    seen = joints_ref.visible(target, visibility)
    tgt = torch.where(seen[..., None], torch.as_tensor(target).to(dt), torch.zeros((), dtype=dt))
    s = ((_select(joints, canon, Jc) - tgt) ** 2).sum(-1)
    s2 = float(robust_scale) ** 2
    rho = 2.0 * s2 * (torch.sqrt(1.0 + s / s2) - 1.0) if robust_scale > 0 else s
    wj = torch.ones(Jc, dtype=dt) if joint_weights is None else torch.as_tensor(joint_weights).to(dt)
    bw = fit_ref.window_sizes(N, window).to(dt)[:, None]
    return float(w_k3d) * (seen.to(dt) * wj[None] * rho / (3.0 * Jc * bw)).sum()


def oracle_joints(t, betas, pose, trans, log_beta_scales, betas_trans, mask, dtype=F64):
    """``joints_ref.oracle_joints`` with the dense oracle evaluated in ``dtype`` (the float32 evaluation measures what a row error can
    resolve)."""
    if dtype == F64:
        return joints_ref.oracle_joints(t, betas, pose, trans, log_beta_scales, betas_trans, mask)
    N = pose.shape[0]
    m = lbs_ref64.dense_model(t, dtype)
    ex = lambda x: None if x is None else x[None].expand(N, *x.shape)  # noqa: E731
    o = lbs_ref.smal_forward(m, betas[None].expand(N, -1), pose * torch.as_tensor(mask).to(dtype), trans=None, betas_logscale=ex(log_beta_scales),
                             betas_trans=ex(betas_trans), propagate_scaling=False, allow_limb_scaling=True)
    return o["joints"] + trans[:, None]


def fit_eval(t, params, mask, cams, S, target, visibility, confidence, joint_weights, canon, w_k2d, robust_scale_px, window, w_k3d=0.0,
             robust_scale=0.0, target3d=None, visibility3d=None, dtype=F64):
    """``oracle joints -> 2-D term (+ 3-D term)`` on float32 parameters.  Returns a dict: ``term2d``, ``term3d`` (0 when not asked for),
    ``joints (N,J,3)``, ``yx (N,Nv,Jc,2)``, ``seen (N,Nv,Jc)`` and ``grads`` of the sum of the terms on betas, pose (with respect to the
    MASKED pose), trans, log_beta_scales, betas_trans - all in ``dtype``."""
    leaves = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    masked = leaves["pose"] * torch.as_tensor(mask).to(dtype)
    masked.retain_grad()
    joints = oracle_joints(t, leaves["betas"], masked, leaves["trans"], leaves.get("log_beta_scales"), leaves.get("betas_trans"),
                           torch.ones_like(torch.as_tensor(mask)), dtype)
    zero = torch.zeros((), dtype=dtype)
    term2d, yx, seen = kp2d_term(joints, cams, S, target, visibility, confidence, joint_weights, canon, w_k2d, robust_scale_px, window,
                                 with_projection=True)
    if not w_k2d > 0:
        term2d = zero
    term3d = zero
    if target3d is not None and w_k3d > 0:
        term3d = kp3d_term(joints, target3d, visibility3d, joint_weights, canon, w_k3d, robust_scale, window)
    total = term2d + term3d
    if total.requires_grad:
        total.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in leaves.items() if k != "pose"}
    grads["pose"] = torch.zeros_like(masked) if masked.grad is None else masked.grad.detach()
    return dict(term2d=term2d.detach(), term3d=term3d.detach(), joints=joints.detach(), yx=yx, seen=seen, grads=grads)
