"""The fused multi-view 2-D keypoint evaluation (smil_kp2d_fit_eval, smilify_amd/csrc/joints.hip) and ``KeypointFitter2D`` against float64:
``tests/kp2d_ref.py`` (dense-LBS oracle joints -> float64 projection -> the term, gradients by autograd), ``fit_ref.priors_and_temporal`` and
``fit_ref.adam``.  The problems are those of ``tests/kp2d_cases.py``; ``tests/test_kp2d_ref_cpu.py`` checks on the CPU that every one of
them resolves a row error of TOL / 16.

Bounds
* objs[0], objs[9]: relative 2e-5 (``OBJ_RTOL`` of tests/test_gpu_fit_keypoints3d.py);
* gradients: ``row_err <= lbs_ref64.TOL`` of d_theta (d_pose), d_trans, d_beta, d_logscale, d_btrans; ``yx_out``: TOL["yx"]; ``joints``:
  TOL["joints"]; a frame with nothing seen: every gradient bit zero;
* against ``SMALFitter``: objs[0] 1e-4 relative (the project's loss parity), each gradient within the SUM of the two paths' TOL (each path
  is within its own bound of the same float64 reference);
* trajectory: the rule of tests/test_gpu_fit_keypoints3d.py - the error against the float64 trajectory, max-abs and RMS, at most 4 x that of
  the float32 ``torch.optim.Adam`` yardstick, floored at 2^-24 max|value| for tensors of fewer than 64 elements.
Every test prints what it measured.
"""
import pytest
import torch

import fit_ref
import joints_cases
import kp2d_cases
import kp2d_ref
from lbs_ref64 import TOL, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
OBJ_RTOL = 2e-5
W_K2D = 25.0  # the reference's stage-0 joint weight (OPT_WEIGHTS column 0)
GRADS = (("d_theta", "pose"), ("d_trans", "trans"), ("d_beta", "betas"), ("d_logscale", "log_beta_scales"), ("d_btrans", "betas_trans"))


def _fitter(t, p, sigma_px=0.0, weights=True, with_3d=False, sigma=0.0, train_tables=True):
    from smilify_amd.fit_keypoints2d import KeypointFitter2D

    from smilify_amd.cameras import FoVCameras

    c = p["cams"]
    cams = dict(R=c["R"], T=c["T"], fov=c["fov"], aspect_ratio=c.get("aspect"), principal_point=c.get("principal"))
    if p["views"] == 1:  # (the other form the constructor takes)
        cams = FoVCameras(c["R"], c["T"], c["fov"], c.get("aspect"), principal_point=c.get("principal"))
    train_ls, train_bt = train_tables if isinstance(train_tables, tuple) else (train_tables, train_tables)
    f = KeypointFitter2D(DEV, p["target"], p["vis"] if weights else None, cameras=cams, image_size=p["S"],
                         confidence=p["conf"] if weights else None, target_keypoints_3d=p["target3d"] if with_3d else None,
                         visibility_3d=p["vis3d"] if (with_3d and weights) else None, tables=t, canonical_joints=p["canon"],
                         joint_weights=p["wj"] if weights else None, robust_scale_px=sigma_px, robust_scale=sigma)
    with torch.no_grad():
        f.betas.copy_(p["params"]["betas"])
        f._pose.copy_(p["params"]["pose"])
        f.trans.copy_(p["params"]["trans"])
        f.log_beta_scales.copy_(p["params"]["log_beta_scales"])
        f.betas_trans.copy_(p["params"]["betas_trans"])
        f.global_mask.copy_(p["mask"][:1])
        f.rotation_mask.copy_(p["mask"][1:])
    f.log_beta_scales.requires_grad_(train_ls)
    f.betas_trans.requires_grad_(train_bt)
    return f


def _kernel_joints(f, weights, window):
    """``joints_out (N,J,3)`` of smil_kp2d_fit_eval itself, from a launch with the term weights of the case (no gradient output)."""
    from smilify_amd import _lib, engine

    N, J = f.num_images, f.tables.J
    cfg = engine.fit_config(N, J, f.n_betas, window, (0.0,) * 6, 0.0, limit=f.config.JOINT_LIMIT)
    out = torch.full((N, J, 3), float("nan"), device=DEV)
    ls, bt = f._scale_tables()
    f._term_eval(cfg, weights, f.betas.detach().contiguous(), f.trans.detach().contiguous(), ls, bt, f._mask_table(),
                 torch.zeros(_lib.N_OBJS, device=DEV), None, None, None, None, None, joints_out=out)
    return out


def _zero_bits(x):
    return not x.contiguous().view(torch.int32).any()


def _yx_err(got, want, N):
    """Row error of the projections where the reference is finite; the NaN pattern must agree exactly."""
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(got.cpu())), "yx_out: the NaN pattern differs from the depth rule"
    return row_err(torch.where(fin, got.cpu(), torch.zeros(())), torch.where(fin, want, torch.zeros((), dtype=want.dtype)), N)


def _compare(name, f, p, ref, objs, got, N, keys=GRADS, weights=(W_K2D, 0.0), window=3):
    """objs[0], the kernel's ``joints_out`` (every frame, the dead ones too) and ``yx_out`` and the gradients against the reference
    ``ref``; prints the figures, then asserts."""
    want_pose = ref["grads"]["pose"] * p["mask"].double()  # (after smil_prior_losses: the gradient on the parameter)
    rel = abs(objs[0].item() - ref["term2d"].item()) / abs(ref["term2d"].item())
    yx, joints_p = f.project(return_joints=True)
    joints_k = _kernel_joints(f, weights, window)
    assert torch.equal(joints_k, joints_p), "joints_out differs between two launches"
    errs = dict(joints=row_err(joints_k, ref["joints"], N), yx=_yx_err(yx, ref["yx"], N))
    for k, n in keys:
        if got[n] is not None:
            errs[k] = row_err(got[n], want_pose if n == "pose" else ref["grads"][n], N if n in ("pose", "trans") else 1)
    print(f"[kp2d] {name}: objs[0] rel {rel:.1e} " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert rel <= OBJ_RTOL, (name, objs, ref["term2d"])
    for k, e in errs.items():
        assert e <= TOL[k], f"{name}: {k} row error {e:.3e} above {TOL[k]:.1e}"
    return errs


@pytest.mark.parametrize("sigma_px", [0.0, 2.0])
@pytest.mark.parametrize("window", [3, 10])
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("key,views,per_image,aspect_pp,seed", kp2d_cases.GPU_PROBLEMS)
def test_fused_against_float64(tables, key, views, per_image, aspect_pp, seed, weights, window, sigma_px):
    """N = 7 frames (windows of 3, 3, 1 or one of 7), J = 55, 31 (static), 65 (two joints per lane) and > 128, views 1 and 3, camera tables
    of ``views`` and of ``N * views`` rows, aspect and principal point on and off; confidences, visibility and joint weights on, and off
    together (the NULL paths).  The problem holds a NaN target row, an entry with visibility 0, confidences 0 and NaN, a residual of 350
    px, a frame behind camera 0 (unseen there, seen in the other views) and a frame with nothing seen."""
    t = joints_cases.get_model(key, tables)
    N = 7
    p = kp2d_cases.problem(t, N, views, seed, per_image, aspect_pp)
    ref = kp2d_cases.reference(t, p, W_K2D, sigma_px, window, weights)
    f = _fitter(t, p, sigma_px, weights)
    objs, got = f.loss_and_grads(W_K2D, window=window)  # (no priors: prior_losses only applies mask and train flags)
    name = f"fused[{key}-v{views}-img{int(per_image)}-pp{int(aspect_pp)}-w{int(weights)}-win{window}-sigma{sigma_px}]"
    assert not objs[1:].any(), (name, objs)  # objs[1:9] untouched, objs[9] too: no 3-D term was asked for
    _compare(name, f, p, ref, objs, got, N, window=window)
    n = p["dead_frame"]
    assert _zero_bits(got["pose"][n]) and _zero_bits(got["trans"][n]), f"{name}: the frame with nothing seen has a gradient"
    b = p["behind_frame"]
    seen = f.seen().cpu()
    assert torch.equal(seen, ref["seen"]) and not seen[b, 0].any() and (views == 1 or bool(seen[b, 1:].all()))
    if views == 1:  # behind its only camera: dead too
        assert _zero_bits(got["pose"][b]) and _zero_bits(got["trans"][b])
    err = f.reprojection_errors().cpu()
    want = torch.where(ref["seen"], (ref["yx"] - p["target"].double()).norm(dim=-1), torch.full((), float("nan"), dtype=torch.float64))
    assert torch.equal(torch.isnan(err), ~ref["seen"])
    assert bool(((err.double() - want)[ref["seen"]].abs() <= 1e-6 * want[ref["seen"]].abs() + 1e-4).all())  # (float32 pixels of ~1e2)


@pytest.mark.parametrize("kw", kp2d_cases.BOTH_PROBLEMS, ids=lambda kw: kw["key"])
@pytest.mark.parametrize("weights", [True, False])
def test_both_terms(tables, kw, weights):
    """The 3-D term in the same launch: objs[0] and objs[9] each against their own reference, the gradients against the reference of the
    sum (the weights make the two terms of one size); the frame that is dead in 2-D is visible in 3-D and has a gradient."""
    kw = dict(kw)
    key = kw.pop("key")
    t = joints_cases.get_model(key, tables)
    N, window, sigma_px, sigma = kw["N"], 3, 2.0, 0.05
    p = kp2d_cases.problem(t, kw.pop("N"), kw.pop("views"), kw.pop("seed"), **kw)
    w_k3d = 2e6 / p["length"] ** 2
    ref = kp2d_cases.reference(t, p, W_K2D, sigma_px, window, weights, w_k3d=w_k3d, sigma=sigma)
    f = _fitter(t, p, sigma_px, weights, with_3d=True, sigma=sigma)
    objs, got = f.loss_and_grads(W_K2D, w_k3d, window=window)
    rel3 = abs(objs[9].item() - ref["term3d"].item()) / abs(ref["term3d"].item())
    print(f"[kp2d] both[{key}-w{int(weights)}]: term2d {ref['term2d'].item():.4e} term3d {ref['term3d'].item():.4e} objs[9] rel {rel3:.1e}")
    assert not objs[1:9].any() and rel3 <= OBJ_RTOL, objs
    assert 0.05 < ref["term3d"].item() / ref["term2d"].item() < 20.0
    _compare(f"both[{key}-w{int(weights)}]", f, p, ref, objs, got, N, weights=(W_K2D, w_k3d), window=window)
    n = p["dead_frame"]
    assert got["pose"][n].any() and got["trans"][n].any() and ref["grads"]["trans"][n].any()
    only3 = kp2d_cases.reference(t, p, 0.0, sigma_px, window, weights, w_k3d=w_k3d, sigma=sigma)  # w_k2d = 0: the 3-D term alone
    objs3, got3 = f.loss_and_grads(0.0, w_k3d, window=window)
    assert objs3[0].item() == 0.0 and abs(objs3[9].item() - only3["term3d"].item()) <= OBJ_RTOL * only3["term3d"].item()
    e = row_err(got3["trans"], only3["grads"]["trans"], N)
    assert e <= TOL["d_trans"], e


@pytest.mark.parametrize("key,views,per_image,aspect_pp,seed", kp2d_cases.GPU_PROBLEMS[:4])
def test_fused_equals_unfused(tables, key, views, per_image, aspect_pp, seed):
    """Against ``SMAL.joints`` -> the float64 projection and term as a torch expression on the device -> ``backward()``."""
    from smilify_amd.smal_torch import SMAL

    t = joints_cases.get_model(key, tables)
    N, window, sigma_px = 7, 3, 2.0
    p = kp2d_cases.problem(t, N, views, seed, per_image, aspect_pp)
    f = _fitter(t, p, sigma_px)
    objs, got = f.loss_and_grads(W_K2D, window=window)
    smal = SMAL(DEV, tables=t)
    mask = p["mask"].to(DEV)
    leaf = {k: v.to(DEV).clone().requires_grad_() for k, v in p["params"].items()}
    masked = leaf["pose"] * mask
    masked.retain_grad()
    j = smal.joints(leaf["betas"][None], masked, None, leaf["log_beta_scales"], leaf["betas_trans"]).double() + leaf["trans"].double()[:, None]
    unfused = kp2d_ref.kp2d_term(j, p["cams"], p["S"], p["target"], p["vis"], p["conf"], p["wj"], p["canon"], W_K2D, sigma_px, window)
    unfused.backward()
    rel = abs(unfused.item() - objs[0].item()) / abs(unfused.item())
    errs = {}
    for k, a, b, rows in (("d_theta", got["pose"], masked.grad * mask, N), ("d_trans", got["trans"], leaf["trans"].grad, N),
                          ("d_beta", got["betas"], leaf["betas"].grad, 1), ("d_logscale", got["log_beta_scales"], leaf["log_beta_scales"].grad, 1),
                          ("d_btrans", got["betas_trans"], leaf["betas_trans"].grad, 1)):
        errs[k] = row_err(a, b, rows)
    print(f"[kp2d] unfused[{key}-v{views}]: objs[0] rel {rel:.1e} " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert rel <= OBJ_RTOL
    for k, e in errs.items():
        assert e <= TOL[k], f"fused and unfused {k} differ by {e:.3e}"


@pytest.mark.parametrize("key,N,views,per_image,seed", kp2d_cases.BLOCK_PROBLEMS)
def test_block_loop_and_view_cap(tables, key, N, views, per_image, seed):
    """The mouse at one block's frames - 1, exactly that and + 1, and at 4099 frames with two views (1024 blocks loop, the last round is
    ragged); three joints under 64 views (the cap) with the cameras staged per block and per frame.  The three-joint tube's joints do
    not depend on the log scales beyond rounding (its float64 d_logscale is a cancelled row): that table is frozen there, ``betas_trans``
    is trained (a shared table's sum columns beside 8 KB of staged cameras)."""
    t = joints_cases.get_model(key, tables)
    window, sigma_px = 3, 2.0
    p = kp2d_cases.problem(t, N, views, seed, per_image, True)
    ref = kp2d_cases.reference(t, p, W_K2D, sigma_px, window)
    f = _fitter(t, p, sigma_px, train_tables=(key != "j3", True))
    objs, got = f.loss_and_grads(W_K2D, window=window)
    assert not objs[1:].any()
    _compare(f"block[{key}-N{N}-v{views}-img{int(per_image)}]", f, p, ref, objs, got, N)


@pytest.mark.parametrize("sigma_px", [0.0, 2.0])
def test_one_joint_behind_one_camera(tables, sigma_px):
    """The static three-joint tube with its last joint carried past camera 1 by a ``betas_trans`` row (z_view < -0.1 there, in every
    frame) while the other two joints stay in front: within (frame, view 1) that entry alone is unseen and NaN in ``yx_out``, and it is
    seen in views 0 and 2 - the depth test is taken per entry."""
    t = joints_cases.get_model("j3_static", tables)
    p = kp2d_cases.single_joint_problem(t, kp2d_cases.SINGLE_JOINT_SEED)
    N, window = p["N"], 3
    ref = kp2d_cases.reference(t, p, W_K2D, sigma_px, window)
    f = _fitter(t, p, sigma_px)
    objs, got = f.loss_and_grads(W_K2D, window=window)
    assert not objs[1:].any()
    _compare(f"one-joint[sigma{sigma_px}]", f, p, ref, objs, got, N, window=window)
    seen, yx = f.seen().cpu(), f.project().cpu()
    want = torch.ones(N, 3, 3, dtype=torch.bool)
    want[:, 1, 0] = False  # (canon[0] is the joint that was moved)
    assert torch.equal(seen, want) and torch.equal(seen, ref["seen"]) and torch.equal(torch.isnan(yx).any(-1), ~want)


def _raw_call(f, cam, cfg_N=None):
    """smil_kp2d_fit_eval through ctypes with a hand-built ``SmilCameras``: (return code, smil_last_error)."""
    import ctypes

    from smilify_amd import _lib, engine

    lib = _lib.load()
    N, J = f.num_images, f.tables.J
    cfg = engine.fit_config(N if cfg_N is None else cfg_N, J, f.n_betas, 3, (0.0,) * 6)
    betas, trans = f.betas.detach().contiguous(), f.trans.detach().contiguous()
    i = engine._joints_inputs(f.joint_tables, betas, f._pose, trans, None, None, None, dict(trans_after_joints=True))
    objs = torch.zeros(_lib.N_OBJS, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    rc = lib.smil_kp2d_fit_eval(ctypes.byref(cfg), W_K2D, 0.0, ctypes.byref(f.joint_tables.struct), ctypes.byref(i), ctypes.byref(cam),
                                int(f.canonical_joints.numel()), ptr(f.canonical_joints), ptr(f.target_keypoints_2d), None, None, None, 0.0,
                                0.0, None, None, ptr(objs), None, None, None, None, None, None, None, ptr(ws), None)
    torch.cuda.synchronize()
    return rc, lib.smil_last_error().decode()


def test_reproducible_and_bad_arguments(tables):
    from smilify_amd import _lib
    from smilify_amd.fit_keypoints2d import KeypointFitter2D

    t = joints_cases.get_model("stick", tables)
    p = kp2d_cases.problem(t, 7, 3, 7, per_image=True, with_3d=True)
    f = _fitter(t, p, 2.0, with_3d=True, sigma=0.05)
    (o1, g1), (o2, g2) = f.loss_and_grads(W_K2D, 40.0, window=3), f.loss_and_grads(W_K2D, 40.0, window=3)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert torch.equal(f.project().view(torch.int32), f.project().view(torch.int32))  # (bits: the frame behind camera 0 holds NaN)
    with pytest.raises(_lib.SmilError, match="smil_kp2d_fit_eval"):
        f.loss_and_grads(float("nan"))
    with pytest.raises(_lib.SmilError, match="smil_kp2d_fit_eval"):
        f.loss_and_grads(-1.0)
    with pytest.raises(_lib.SmilError, match="neither term"):
        f.loss_and_grads(0.0, 0.0)
    c = p["cams"]
    kw = dict(image_size=p["S"], tables=t, canonical_joints=p["canon"])
    with pytest.raises(_lib.SmilError, match="views"):
        KeypointFitter2D(DEV, torch.zeros(2, 65, len(p["canon"]), 2), cameras=dict(R=c["R"][:1], T=c["T"][:1], fov=c["fov"][:1]), **kw)
    with pytest.raises(_lib.SmilError, match="rows"):
        KeypointFitter2D(DEV, p["target"], cameras=dict(R=c["R"][:2], T=c["T"][:1], fov=c["fov"][:1]), **kw)
    with pytest.raises(ValueError):
        KeypointFitter2D(DEV, p["target"][..., :1], cameras=dict(R=c["R"], T=c["T"], fov=c["fov"]), **kw)
    with pytest.raises(ValueError):
        KeypointFitter2D(DEV, p["target"], p["vis"][:, :1], cameras=dict(R=c["R"], T=c["T"], fov=c["fov"]), **kw)
    no3d = _fitter(t, p, 0.0)
    with pytest.raises(RuntimeError, match="target_keypoints_3d"):
        no3d.initialise_from_alignment()
    with pytest.raises(ValueError, match="target_keypoints_3d"):
        no3d.loss_and_grads(W_K2D, 1.0)
    status = f.initialise_from_alignment()
    assert status.dtype == torch.int32 and tuple(status.shape) == (7,)
    assert set(f.export_parameters(0)) == {"global_rotation", "joint_rotations", "betas", "trans", "log_betascale", "betas_trans"}
    # engine.CameraSet refuses a table of 2 rows at 3 views in Python ...
    from smilify_amd import engine

    with pytest.raises(_lib.SmilError, match="rows"):
        engine.CameraSet(f.cameras.R[:2].contiguous(), f.cameras.T, f.cameras.fov, None, 3, p["S"]).struct(21)
    # ... and the C entry point's own checks, reached through ctypes with a hand-built SmilCameras (the struct of the fitter's cameras,
    # one field changed at a time); the unchanged struct is accepted
    def cam(**fields):
        s = f.cameras.struct(21)
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    assert _raw_call(f, cam())[0] == 0
    for fields, cfg_N, text in ((dict(views=65, N=7 * 65), None, "views=65 outside 1..64"), (dict(views=0), None, "views=0 outside 1..64"),
                                (dict(N=20), None, "cameras hold N=20 images"), (dict(nR=2), None, "camera table R has 2 rows"),
                                (dict(nFov=2), None, "camera table fov has 2 rows"), (dict(), 6, "cfg holds N=6")):
        rc, msg = _raw_call(f, cam(**fields), cfg_N)
        assert rc != 0 and text in msg, (fields, rc, msg)


@pytest.mark.parametrize("kw", kp2d_cases.SHIPPED_PROBLEMS, ids=lambda kw: f"{kw['key']}-v{kw['views']}")
def test_against_the_shipped_fitter(tables, kw):
    """``SMALFitter(views=Nv)`` with the joint weight alone (stage 0 without its temporal term) on the same parameters, cameras (through
    ``set_cameras`` with ``principal_point``) and targets, zero silhouettes, its per-frame scale tables filled with the shared rows: the
    term and every gradient of the two paths, N = 6, window 3, rho = s, no confidences and no joint weights.  The canonical list holds no
    duplicate here: ``smil_joint_loss`` keeps ONE gradient slot per model joint (a joint named twice keeps the last entry's gradient; measured
    1.8e-2 of d_theta on such a list), which is ``SMALFitter``'s documented input (its lists name every joint once), not this kernel's."""
    from smilify_amd.config import FitterConfig
    from smilify_amd.fitter import SMALFitter

    kw = dict(kw)
    key, views = kw.pop("key"), kw["views"]
    t = joints_cases.get_model(key, tables)
    N, window, S = kw["N"], 3, kw["size"]
    p = kp2d_cases.problem(t, kw.pop("N"), kw.pop("views"), kw.pop("seed"), **kw)
    ref = kp2d_cases.reference(t, p, W_K2D, 0.0, window, weights=False)
    seen = ref["seen"]
    f = _fitter(t, p, 0.0, weights=False)
    objs, got = f.loss_and_grads(W_K2D, window=window)
    n_img, Jc = N * views, len(p["canon"])
    tj = torch.where(torch.isfinite(p["target"]), p["target"], torch.zeros(())).reshape(n_img, Jc, 2)
    data = (torch.zeros(n_img, 3, S, S), torch.zeros(n_img, 1, S, S), tj, seen.reshape(n_img, Jc).long())
    s = SMALFitter(DEV, data, N, -1, False, tables=t, config=FitterConfig.from_tables(t, WINDOW_SIZE=window, CANONICAL_MODEL_JOINTS=p["canon"]),
                   views=views)
    c = p["cams"]
    s.set_cameras(c["R"].to(DEV), c["T"].to(DEV), fov=c["fov"].to(DEV), aspect_ratio=c["aspect"].to(DEV), principal_point=c["principal"].to(DEV))
    with torch.no_grad():
        s.betas.copy_(p["params"]["betas"])
        s._pose.copy_(p["params"]["pose"])
        s.trans.copy_(p["params"]["trans"])
        s.log_beta_scales.copy_(p["params"]["log_beta_scales"][None].expand(N, -1, -1))
        s.betas_trans.copy_(p["params"]["betas_trans"][None].expand(N, -1, -1))
        s.global_mask.copy_(p["mask"][:1])
        s.rotation_mask.copy_(p["mask"][1:])
    s.log_beta_scales.requires_grad = True
    s.betas_trans.requires_grad = True
    s.fov.requires_grad = False
    objs_s, got_s = s._loss_and_grads(None, (W_K2D, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0, window=window)
    rel = abs(objs[0].item() - objs_s[0].item()) / abs(objs_s[0].item())
    errs = {}
    for k, n in GRADS:
        a, b = got[n], got_s[n]
        if a is None or (n == "betas" and t.nB == 0):
            continue
        b = b.sum(0) if n in ("log_beta_scales", "betas_trans") else b
        errs[k] = row_err(a, b.reshape(a.shape), N if n in ("pose", "trans") else 1)
    print(f"[kp2d] shipped[{key}-v{views}]: objs[0] {objs[0].item():.6e} / {objs_s[0].item():.6e} rel {rel:.1e} " +
          " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert rel <= 1e-4
    assert abs(objs[0].item() - ref["term2d"].item()) <= OBJ_RTOL * ref["term2d"].item()
    for k, e in errs.items():
        assert e <= 2 * TOL[k], f"{k}: the two paths differ by {e:.3e}, above the sum of their bounds {2 * TOL[k]:.1e}"


def _trajectory64(t, p, sigma_px, sigma, weights, window, train, steps, lr, dtype):
    """``steps`` iterations of oracle gradients + priors + Adam.  dtype float64: the reference trajectory; float32: the yardstick (the
    float64 gradients of the float32 parameters, rounded, stepped by torch.optim.Adam in float32)."""
    w_k2d, w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp = weights
    names = [k for k in ("betas", "pose", "trans", "log_beta_scales", "betas_trans") if train.get(k, True)]
    cur = {k: v.to(dtype).clone() for k, v in p["params"].items()}
    state, opt = {}, None
    if dtype == torch.float32:
        leaves = {k: cur[k].requires_grad_() for k in names}
        opt = torch.optim.Adam([leaves[k] for k in names], lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    for step in range(1, steps + 1):
        vals = {k: v.detach() for k, v in cur.items()}
        g = kp2d_cases.reference(t, dict(p, params=vals), w_k2d, sigma_px, window, True, w_k3d=w_k3d, sigma=sigma)["grads"]
        pr = fit_ref.priors_and_temporal(vals["pose"], vals["trans"], vals["betas"], torch.zeros(t.nB), torch.eye(t.nB), p["mask"],
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


@pytest.mark.parametrize("key,stage0", [("synthetic", True), ("stick", False)])
def test_trajectory(tables, key, stage0):
    """Five fit_steps at N = 6 (windows of 4 and 2), two views, both terms and every prior and temporal weight on, against the float64
    trajectory: once with the stage-0 flags (joint_rotations and the scale tables frozen), once with everything trained."""
    t = joints_cases.get_model(key, tables)
    N, views, steps, lr, window, sigma_px, sigma = 6, 2, 5, 5e-3, 4, 2.0, 0.05
    p = kp2d_cases.problem(t, N, views, 200 + stage0, per_image=True, with_3d=True)
    weights = (W_K2D, 2e6 / p["length"] ** 2, 1.5, 2.0, 100.0, 0.1, 30.0)  # w_k2d, w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp
    train = dict(joints=not stage0, log_beta_scales=not stage0, betas_trans=not stage0)
    train["global"] = True
    f = _fitter(t, p, sigma_px, with_3d=True, sigma=sigma, train_tables=not stage0)
    f.joint_rotations.requires_grad_(not stage0)
    f.betas_prec = torch.eye(t.nB, device=DEV)  # (the identity fallback; STICK ships a covariance)
    f.mean_betas = torch.zeros(t.nB, device=DEV)
    f.begin_stage(lr)
    for _ in range(steps):
        objs = f.fit_step(*weights, window=window)
    assert objs.shape == (10,) and objs.is_cuda and bool(torch.isfinite(objs).all()) and objs[0] > 0 and objs[9] > 0
    got = dict(betas=f.betas, pose=f._pose, trans=f.trans, log_beta_scales=f.log_beta_scales, betas_trans=f.betas_trans)
    args = (t, p, sigma_px, sigma, weights, window, train, steps, lr)
    ref, yard = _trajectory64(*args, torch.float64), _trajectory64(*args, torch.float32)
    missed = []
    for k in got:
        if ref[k].numel() == 0:
            continue
        e_k, e_y = (got[k].detach().cpu().double() - ref[k]).abs(), (yard[k] - ref[k]).abs()
        if not train.get(k, True):
            assert torch.equal(got[k].detach().cpu(), p["params"][k]), f"{k} is frozen but moved"
            continue
        floor = U * ref[k].abs().max().item() if ref[k].numel() < 64 else 0.0
        y_max, y_rms = max(e_y.max().item(), floor), max(e_y.pow(2).mean().sqrt().item(), floor)
        k_max, k_rms = e_k.max().item(), e_k.pow(2).mean().sqrt().item()
        print(f"[kp2d] trajectory[{key}] {k}: kernel max {k_max:.3e} rms {k_rms:.3e}; float32 yardstick max {y_max:.3e} rms {y_rms:.3e}")
        if not (k_max <= 4 * y_max and k_rms <= 4 * y_rms):
            missed.append((k, k_max, y_max, k_rms, y_rms))
        assert (ref[k] - p["params"][k].double()).abs().max() > 0.5 * lr, f"{k} did not move"
    if stage0:
        assert torch.equal(f._pose[:, 1:].cpu(), p["params"]["pose"][:, 1:]), "joint_rotations are frozen but moved"
    assert not missed, f"(parameter, kernel max, yardstick max, kernel rms, yardstick rms) beyond 4 x the yardstick: {missed}"
