"""The fused 3-D keypoint evaluation (smil_kp3d_fit_eval, smilify_amd/csrc/joints.hip) and ``KeypointFitter3D`` against float64:
``tests/joints_ref.py`` (dense-LBS oracle joints -> the term, gradients by autograd), ``fit_ref.priors_and_temporal`` and ``fit_ref.adam``.

Bounds
* objs[9]: relative 2e-5, what tests/test_gpu_fit_kernels.py asks of a reduced objective below its grid cap;
* gradients: ``row_err <= lbs_ref64.TOL`` of d_theta (d_pose), d_trans, d_beta, d_logscale, d_btrans; a frame with nothing visible:
  every gradient bit zero;
* trajectory: the bounds tests/test_gpu_fit_kernels.py gives the Adam step - the error against the float64 trajectory of every
  parameter, max-abs and RMS, at most 4 x that of the float32 yardstick (float64 gradients of the float32 parameters, rounded, stepped
  by ``torch.optim.Adam`` in float32 on the CPU), the yardstick floored at 2^-24 max|value| for tensors of fewer than 64 elements;
* ``initialise_from_alignment``: the float64 composition (oracle joints -> ``align_ref.rigid_transform`` -> the new global rotation
  and translation, rounded to the float32 the parameters are stored in -> oracle joints) misses the float32 targets by a row error of
  6.2e-8 (measured on the CPU, printed by the test; written 8e-8 by ``lbs_ref64``'s rounding-up rule); with the factor 16 of its
  margin policy the bound is 1.28e-6, on the
  joints and on the recovered rotation matrix and translation alike.
"""
import pytest
import torch

import align_ref
import fit_ref
import joints_cases
import joints_ref
import rotations_ref
from lbs_ref64 import TOL, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
OBJ_RTOL = 2e-5
INIT_MEASURED, INIT_MARGIN = 8e-8, 16


def _problem(t, N, seed, Jc=None, train_tables=True):
    """float32 parameters, a permuted strict subset of the joints, and targets near the posed joints with a sentinel row, a NaN row,
    a frame with nothing visible and one residual far beyond any sigma."""
    g = torch.Generator().manual_seed(seed)
    J, nB = t.J, t.nB
    Jc = max(2, (2 * J) // 3) if Jc is None else Jc
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    params = dict(betas=0.4 * rn(nB), pose=0.3 * rn(N, J, 3), trans=0.1 * rn(N, 3), log_beta_scales=0.05 * rn(J, 3), betas_trans=0.02 * rn(J, 3))
    mask = (torch.rand(J, 3, generator=g) < 0.8).float()
    canon = torch.randperm(J, generator=g)[:Jc].tolist()
    joints = joints_ref.oracle_joints(t, *(params[k].double() for k in ("betas", "pose", "trans", "log_beta_scales", "betas_trans")), mask)
    target = (joints[:, canon] + 0.05 * rn(N, Jc, 3).double()).float()
    target[0, 1] = 0.0
    target[1, 0, 2] = float("nan")
    target[2] = 0.0
    target[3, :, 0] = float("inf")
    target[N - 1, Jc - 1] += 5.0
    vis = torch.ones(N, Jc, dtype=torch.uint8)
    vis[0, 0] = 0
    wj = (0.5 + torch.rand(Jc, generator=g)).double()
    wj[Jc // 2] = 0.0
    return params, mask, canon, target, vis, wj


def _fitter(t, params, mask, canon, target, vis, wj, sigma, train_tables=True):
    from smilify_amd.fit_keypoints3d import KeypointFitter3D

    f = KeypointFitter3D(DEV, target, vis, tables=t, canonical_joints=canon, joint_weights=wj, robust_scale=sigma)
    with torch.no_grad():
        f.betas.copy_(params["betas"])
        f._pose.copy_(params["pose"])
        f.trans.copy_(params["trans"])
        f.log_beta_scales.copy_(params["log_beta_scales"])
        f.betas_trans.copy_(params["betas_trans"])
        f.global_mask.copy_(mask[:1])
        f.rotation_mask.copy_(mask[1:])
    f.log_beta_scales.requires_grad_(train_tables)
    f.betas_trans.requires_grad_(train_tables)
    return f


def _zero_bits(x):
    return not x.contiguous().view(torch.int32).any()


@pytest.mark.parametrize("sigma", [0.0, 0.02])
@pytest.mark.parametrize("window", [3, 10])
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("key", ["stick", "mouse"])
def test_fused_against_float64(tables, key, weights, window, sigma):
    t = joints_cases.get_model(key, tables)
    N, w_k3d = 7, 40.0
    params, mask, canon, target, vis, wj = _problem(t, N, 100 + len(key))
    wj = wj if weights else None
    vis_arg = vis if weights else None  # (visibility and weights absent together: the NULL paths)
    term, joints, grads = joints_ref.fit_eval(t, params, mask, target, vis_arg, wj, canon, w_k3d, sigma, window)
    f = _fitter(t, params, mask, canon, target, vis_arg, wj, sigma)
    objs, got = f.loss_and_grads(w_k3d, window=window)  # (no priors: prior_losses only applies mask and train flags)
    name = f"kp3d[{key}-w{int(weights)}-win{window}-sigma{sigma}]"
    rel = abs(objs[9].item() - term.item()) / abs(term.item())
    assert not objs[:9].any() and rel <= OBJ_RTOL, (name, objs, term)
    want_pose = grads["pose"] * mask.double()  # (after smil_prior_losses: the gradient on the parameter)
    errs = dict(joints=row_err(f.joints(), joints, N), d_theta=row_err(got["pose"], want_pose, N), d_trans=row_err(got["trans"], grads["trans"], N),
                d_beta=row_err(got["betas"], grads["betas"], 1), d_logscale=row_err(got["log_beta_scales"], grads["log_beta_scales"], 1),
                d_btrans=row_err(got["betas_trans"], grads["betas_trans"], 1))
    print(f"[kp3d] {name}: objs[9] rel {rel:.1e} " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= TOL[k], f"{name}: {k} row error {e:.3e} above {TOL[k]:.1e}"
    for n in (2, 3):  # nothing visible (all sentinel; a non-finite entry in every row): every gradient bit zero
        assert _zero_bits(got["pose"][n]) and _zero_bits(got["trans"][n]), f"{name}: frame {n} has a gradient"

    # fused equals unfused: SMAL.joints -> the term as a torch expression -> backward()
    from smilify_amd.smal_torch import SMAL

    smal = SMAL(DEV, tables=t)
    leaf = {k: v.to(DEV).clone().requires_grad_() for k, v in params.items()}
    masked = leaf["pose"] * mask.to(DEV)
    masked.retain_grad()
    j = smal.joints(leaf["betas"][None], masked, None, leaf["log_beta_scales"], leaf["betas_trans"]).double() + leaf["trans"].double()[:, None]
    tg, seen = target.to(DEV), joints_ref.visible(target, vis_arg).to(DEV)
    s = ((j[:, canon] - torch.where(seen[..., None], tg.double(), torch.zeros((), dtype=torch.float64, device=DEV))) ** 2).sum(-1)
    rho = s if sigma == 0 else 2 * sigma ** 2 * (torch.sqrt(1 + s / sigma ** 2) - 1)
    wj_d = torch.ones(len(canon), dtype=torch.float64, device=DEV) if wj is None else wj.to(DEV)
    bw = fit_ref.window_sizes(N, window).to(DEV)[:, None]
    unfused = w_k3d * (seen.double() * wj_d[None] * rho / (3.0 * len(canon) * bw)).sum()
    unfused.backward()
    assert abs(unfused.item() - objs[9].item()) <= OBJ_RTOL * abs(term.item())
    for k, a, b, rows in (("d_theta", got["pose"], masked.grad * mask.to(DEV), N), ("d_trans", got["trans"], leaf["trans"].grad, N),
                          ("d_beta", got["betas"], leaf["betas"].grad, 1), ("d_logscale", got["log_beta_scales"], leaf["log_beta_scales"].grad, 1),
                          ("d_btrans", got["betas_trans"], leaf["betas_trans"].grad, 1)):
        e = row_err(a, b, rows)
        assert e <= TOL[k], f"{name}: fused and unfused {k} differ by {e:.3e}"


def test_fused_reproducible_and_bad_arguments(tables):
    from smilify_amd import _lib

    t = joints_cases.get_model("stick", tables)
    params, mask, canon, target, vis, wj = _problem(t, 7, 7)
    f = _fitter(t, params, mask, canon, target, vis, wj, 0.02)
    (o1, g1), (o2, g2) = f.loss_and_grads(40.0, window=3), f.loss_and_grads(40.0, window=3)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    with pytest.raises(_lib.SmilError, match="smil_kp3d_fit_eval"):
        f.loss_and_grads(float("nan"))
    with pytest.raises(ValueError):
        _fitter(t, params, mask, canon + [0], target, vis, wj, 0.0)


def _trajectory64(t, params, mask, canon, target, vis, wj, sigma, weights, window, train, steps, lr, dtype):
    """``steps`` iterations of oracle gradients + priors + Adam.  dtype float64: the reference trajectory; float32: the yardstick (the
    float64 gradients of the float32 parameters, rounded, stepped by torch.optim.Adam in float32)."""
    w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp = weights
    names = [k for k in ("betas", "pose", "trans", "log_beta_scales", "betas_trans") if train.get(k, True)]
    cur = {k: v.to(dtype).clone() for k, v in params.items()}
    state, opt = {}, None
    if dtype == torch.float32:
        leaves = {k: cur[k].requires_grad_() for k in names}
        opt = torch.optim.Adam([leaves[k] for k in names], lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    for step in range(1, steps + 1):
        vals = {k: v.detach() for k, v in cur.items()}
        _, _, g = joints_ref.fit_eval(t, vals, mask, target, vis, wj, canon, w_k3d, sigma, window)
        pr = fit_ref.priors_and_temporal(vals["pose"], vals["trans"], vals["betas"], torch.zeros(t.nB), torch.eye(t.nB), mask,
                                         (0.0, 0.0, w_betas, w_pose, w_limit, w_splay), w_temp, 0.01, window,
                                         train=(train["global"], train["joints"], True), upstream=(g["pose"], g["trans"]))
        grad = dict(betas=g["betas"] + pr["d_betas"], pose=pr["d_pose"], trans=pr["d_trans"], log_beta_scales=g["log_beta_scales"],
                    betas_trans=g["betas_trans"])
        if opt is not None:
            for k in names:
                leaves[k].grad = grad[k].float()
            opt.step()
        else:
            for k in names:
                st = state.get(k, (None, None))
                cur[k], m, v = fit_ref.adam(cur[k], [grad[k]], lr, exp_avg=st[0], exp_avg_sq=st[1], step0=step - 1)[0]
                state[k] = (m, v)
    return {k: v.detach().double() for k, v in cur.items()}


@pytest.mark.parametrize("key,stage0", [("synthetic", True), ("stick", False), ("mouse", True)])
def test_iteration_gradients(tables, key, stage0):
    """``loss_and_grads`` with every weight on at N = 6 (windows of 4 and 2): the ten loss terms and the finished gradients (raw 3-D term
    + priors + temporal, masked, train flags applied) against ``joints_ref`` + ``fit_ref.priors_and_temporal``; stage 0 freezes
    joint_rotations and the scale tables."""
    t = joints_cases.get_model(key, tables)
    N, window, sigma = 6, 4, 0.05
    w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp = 40.0, 1.5, 2.0, 100.0, 0.1, 30.0
    params, mask, canon, target, vis, wj = _problem(t, N, 300 + stage0)
    f = _fitter(t, params, mask, canon, target, vis, wj, sigma, train_tables=not stage0)
    f.joint_rotations.requires_grad_(not stage0)
    objs, got = f.loss_and_grads(w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp, window=window)
    term, _, g = joints_ref.fit_eval(t, params, mask, target, vis, wj, canon, w_k3d, sigma, window)
    pr = fit_ref.priors_and_temporal(params["pose"], params["trans"], params["betas"], f.mean_betas, f.betas_prec, mask,
                                     (0.0, 0.0, w_betas, w_pose, w_limit, w_splay), w_temp, f.config.JOINT_LIMIT, window,
                                     train=(True, not stage0, True), upstream=(g["pose"], g["trans"]))
    want = torch.cat([pr["objs"], term[None]])
    err = (objs.cpu().double() - want).abs()
    assert bool((err <= OBJ_RTOL * want.abs()).all()), (objs, want)
    errs = dict(d_theta=row_err(got["pose"], pr["d_pose"], N), d_trans=row_err(got["trans"], pr["d_trans"], N),
                d_beta=row_err(got["betas"], g["betas"] + pr["d_betas"], 1) if t.nB else 0.0)
    if stage0:
        assert got["log_beta_scales"] is None and got["betas_trans"] is None and not got["pose"][:, 1:].any()
    else:
        errs.update(d_logscale=row_err(got["log_beta_scales"], g["log_beta_scales"], 1), d_btrans=row_err(got["betas_trans"], g["betas_trans"], 1))
    print(f"[kp3d] iteration[{key}-stage0={stage0}]: objs rel {float((err / want.abs().clamp(min=1e-300)).max()):.1e} " +
          " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= TOL[k], f"{k} row error {e:.3e} above {TOL[k]:.1e}"


@pytest.mark.parametrize("key,stage0", [("synthetic", True), ("stick", False)])
def test_trajectory(tables, key, stage0):
    """Five fit_steps with every weight on at N = 6 (windows of 4 and 2) against the float64 trajectory: once with joint_rotations and
    the scale tables frozen (stage 0), once with everything trained.

    The step is smil_adam_step_multi_bc64: with smil_adam_step_multi, whose bias corrections are float32, every parameter ends about
    1.9e-7 from the float64 trajectory whatever its magnitude (5e-3 x the 3e-6 .. 1e-5 by which sqrt(1 - beta2^t) is off at steps
    1 .. 5), 3 .. 16 x the yardstick (max-abs) on these parameters of 0.02 .. 0.4."""
    t = joints_cases.get_model(key, tables)
    N, steps, lr, window, sigma = 6, 5, 5e-3, 4, 0.05
    weights = (40.0, 1.5, 2.0, 100.0, 0.1, 30.0)  # w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp
    params, mask, canon, target, vis, wj = _problem(t, N, 200 + stage0)
    train = dict(global_=True, joints=not stage0, log_beta_scales=not stage0, betas_trans=not stage0)
    train["global"] = train.pop("global_")
    f = _fitter(t, params, mask, canon, target, vis, wj, sigma, train_tables=not stage0)
    f.joint_rotations.requires_grad_(not stage0)
    f.betas_prec = torch.eye(t.nB, device=DEV)  # (the identity fallback; STICK ships a covariance)
    f.mean_betas = torch.zeros(t.nB, device=DEV)
    f.begin_stage(lr)
    for _ in range(steps):
        objs = f.fit_step(*weights, window=window)
    assert objs.shape == (10,) and objs.is_cuda and bool(torch.isfinite(objs).all()) and objs[9] > 0
    got = dict(betas=f.betas, pose=f._pose, trans=f.trans, log_beta_scales=f.log_beta_scales, betas_trans=f.betas_trans)
    args = (t, params, mask, canon, target, vis, wj, sigma, weights, window, train, steps, lr)
    ref, yard = _trajectory64(*args, torch.float64), _trajectory64(*args, torch.float32)
    missed = []
    for k in got:
        e_k, e_y = (got[k].detach().cpu().double() - ref[k]).abs(), (yard[k] - ref[k]).abs()
        if not train.get(k, True):
            assert torch.equal(got[k].detach().cpu(), params[k]), f"{k} is frozen but moved"
            continue
        floor = U * ref[k].abs().max().item() if ref[k].numel() < 64 else 0.0
        y_max, y_rms = max(e_y.max().item(), floor), max(e_y.pow(2).mean().sqrt().item(), floor)
        k_max, k_rms = e_k.max().item(), e_k.pow(2).mean().sqrt().item()
        print(f"[kp3d] trajectory[{key}] {k}: kernel max {k_max:.3e} rms {k_rms:.3e}; float32 yardstick max {y_max:.3e} rms {y_rms:.3e}")
        if not (k_max <= 4 * y_max and k_rms <= 4 * y_rms):
            missed.append((k, k_max, y_max, k_rms, y_rms))
        assert (ref[k] - params[k].double()).abs().max() > 0.5 * lr, f"{k} did not move"
    if stage0:
        assert torch.equal(f._pose[:, 1:].cpu(), params["pose"][:, 1:]), "joint_rotations are frozen but moved"
    assert not missed, f"(parameter, kernel max, yardstick max, kernel rms, yardstick rms) beyond 4 x the yardstick: {missed}"


@pytest.mark.parametrize("n,scale", [(5, 0.02), (257, 0.3), (1000, 1.0)])
def test_adam_bias_corrections_in_double(n, scale):
    """smil_adam_step_multi_bc64 on parameters of size ``scale`` with smooth gradients, ten steps from step 1, against float64 Adam:
    the bound of tests/test_gpu_fit_kernels.py (parameter and both moments, max-abs and RMS, at most 4 x the error of float32
    torch.optim.Adam on the CPU over the same gradients, floored at 2^-24 max|value| below 64 elements)."""
    from smilify_amd import engine

    g = torch.Generator().manual_seed(n)
    lr, steps = 5e-3, 10
    p0 = scale * torch.randn(n, generator=g)
    grads = [(torch.randn(n, generator=g) * (0.1 + torch.rand(n, generator=g))).float() for _ in range(steps)]
    ref = fit_ref.adam(p0, grads, lr)[-1]
    yard = p0.clone().requires_grad_()
    opt = torch.optim.Adam([yard], lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for k, gr in enumerate(grads):
        yard.grad = gr.clone()
        opt.step()
        engine.adam_step_multi_bc64([(p, gr.to(DEV), m, v, lr, k + 1)], 0.5, 0.999, 1e-8)
    st = opt.state[yard]
    for what, got, y, want in (("param", p, yard.detach(), ref[0]), ("exp_avg", m, st["exp_avg"], ref[1]), ("exp_avg_sq", v, st["exp_avg_sq"], ref[2])):
        e_k, e_y = (got.cpu().double() - want).abs(), (y.double() - want).abs()
        floor = U * want.abs().max().item() if n < 64 else 0.0
        y_max, y_rms = max(e_y.max().item(), floor), max(e_y.pow(2).mean().sqrt().item(), floor)
        k_max, k_rms = e_k.max().item(), e_k.pow(2).mean().sqrt().item()
        print(f"[kp3d] adam_bc64[n={n}] {what}: kernel max {k_max:.3e} rms {k_rms:.3e}; float32 torch max {y_max:.3e} rms {y_rms:.3e}")
        assert k_max <= 4 * y_max and k_rms <= 4 * y_rms, (what, k_max, y_max, k_rms, y_rms)


def test_initialise_from_alignment(tables):
    """Targets: the rest-pose joints of a shaped STICK under a known rigid motion per frame.  Afterwards ``joints()`` meets the targets
    and the motion is recovered; a frame with two visible targets keeps its parameters and says so."""
    from smilify_amd import align
    from smilify_amd.fit_keypoints3d import KeypointFitter3D

    t = joints_cases.get_model("stick", tables)
    g = torch.Generator().manual_seed(9)
    N, J = 5, t.J
    betas = 0.3 * torch.randn(t.nB, generator=g)
    ones = torch.ones(J, 3)
    rest = joints_ref.oracle_joints(t, betas.double(), torch.zeros(1, J, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64), None,
                                    None, ones)[0]
    aa = torch.randn(N, 3, generator=g, dtype=torch.float64)
    aa = aa / aa.norm(dim=1, keepdim=True) * torch.tensor([0.3, 1.2, 2.0, 2.9, 0.7], dtype=torch.float64)[:, None]
    R = rotations_ref.axis_angle_to_matrix(aa)
    shift = torch.randn(N, 3, generator=g, dtype=torch.float64)
    target = (rest[None] @ R.transpose(1, 2) + shift[:, None]).float()
    vis = torch.ones(N, J, dtype=torch.uint8)
    vis[4, 2:] = 0  # two visible targets: no rotation is determined
    f = KeypointFitter3D(DEV, target, vis, tables=t)
    with torch.no_grad():
        f.betas.copy_(betas)
    before_pose, before_trans = f._pose.clone(), f.trans.detach().clone()

    # the float64 composition on the float32 inputs: what the rounding of targets and parameters alone costs
    p0 = dict(betas=betas.double(), pose=before_pose.cpu().double(), trans=before_trans.cpu().double())
    src = joints_ref.oracle_joints(t, p0["betas"], p0["pose"], p0["trans"], None, None, ones)
    x, _ = align_ref.rigid_transform(src, target.double(), mask=vis.bool())
    c = rest[0]
    G = x.R @ rotations_ref.axis_angle_to_matrix(p0["pose"][:, 0])
    new_trans = (x.R @ (c + p0["trans"])[..., None])[..., 0] + x.t - c
    pose64 = p0["pose"].clone()
    pose64[:, 0] = rotations_ref.matrix_to_axis_angle(G).float().double()
    j64 = joints_ref.oracle_joints(t, p0["betas"], pose64, new_trans.float().double(), None, None, ones)
    measured = row_err(j64[:4], target[:4], 4)
    bound = INIT_MARGIN * INIT_MEASURED
    print(f"[kp3d] initialise_from_alignment: float64 composition on float32 inputs misses the targets by {measured:.2e} (bound {bound:.1e})")
    assert measured <= INIT_MEASURED  # (the figure the bound is built on stays true)

    status = f.initialise_from_alignment()
    assert status.dtype == torch.int32 and status.cpu().tolist() == [align.OK] * 4 + [align.DEGENERATE]
    e_j = row_err(f.joints()[:4], target[:4], 4)
    R_got = rotations_ref.axis_angle_to_matrix(f.global_rotation.detach().cpu().double())
    e_R = row_err(R_got[:4], R[:4], 4)
    want_trans = (R @ c[:, None])[..., 0] + shift - c
    e_t = row_err(f.trans.detach()[:4], want_trans[:4], 4)
    print(f"[kp3d] initialise_from_alignment: joints {e_j:.2e} rotation {e_R:.2e} translation {e_t:.2e}")
    assert e_j <= bound and e_R <= bound and e_t <= bound
    assert torch.equal(f._pose[4], before_pose[4]) and torch.equal(f.trans.detach()[4], before_trans[4])
    assert torch.equal(f._pose[:, 1:], before_pose[:, 1:])
    keys = set(f.export_parameters(0))
    assert keys == {"global_rotation", "joint_rotations", "betas", "trans", "log_betascale", "betas_trans"}
