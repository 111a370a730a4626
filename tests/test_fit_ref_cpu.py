"""Pin ``tests/fit_ref.py`` (the float64 reference of the loss / optimiser kernels) without a GPU: against the float32
oracle ``oracle/fitter_ref.py`` on seeded inputs, against the term values the real reference produced
(``tests/golden/fitter_*.npz``), against ``torch.optim.Adam`` in float64, and against three identities of its own.

Tolerance of the oracle / golden comparisons: the oracle side is float32, a mean over n entries computed by torch's pairwise
sum; ``F32_RTOL = 1e-5`` (about 170 float32 roundings) covers that and is far below any change of a normaliser."""
import numpy as np
import pytest
import torch

import fit_ref
from conftest import oracle_model
from oracle import fitter_ref

F32_RTOL = 1e-5
LIMIT = float(np.float32(0.01))


def _seeded(N, J, nB, seed, jscale=0.02):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(nB, nB, generator=g)
    return dict(grot=0.5 * torch.randn(N, 3, generator=g), jrot=jscale * torch.randn(N, J - 1, 3, generator=g),
                trans=0.2 * torch.randn(N, 3, generator=g), betas=torch.randn(nB, generator=g), mean_b=0.1 * torch.randn(nB, generator=g),
                prec=torch.tril(A) + 2.0 * torch.eye(nB), gmask=torch.tensor([[1.0, 0.0, 1.0]]),
                rmask=(torch.rand(J - 1, 3, generator=g) > 0.2).float())


def _ref(d, weights, w_temp, window, **kw):
    pose = torch.cat([d["grot"][:, None], d["jrot"]], 1)
    return fit_ref.priors_and_temporal(pose, d["trans"], d["betas"], d["mean_b"], d["prec"], torch.cat([d["gmask"], d["rmask"]], 0),
                                       weights, w_temp, LIMIT, window, **kw)


def _oracle_priors(model, d, weights, w_temp, window):
    """The oracle itself, in float32: ``fit_losses`` window by window on a real model (it skins the mesh on the way; with w_j2d = w_reproj
    = 0 it needs no targets and renders nothing) and ``temporal``, with one backward over their sum."""
    N, J = d["grot"].shape[0], d["jrot"].shape[1] + 1
    w = window if window > 0 else N
    P = dict(global_rotation=d["grot"].clone().requires_grad_(), joint_rotations=d["jrot"].clone().requires_grad_(),
             trans=d["trans"].clone().requires_grad_(), betas=d["betas"].clone().requires_grad_(),
             log_beta_scales=torch.zeros(1, J, 3), betas_trans=torch.zeros(1, J, 3), fov=torch.tensor([60.0]))
    cams = dict(R=torch.eye(3)[None], T=torch.tensor([[0.0, 0.0, 3.0]]))
    objs = dict(limit=0.0, pose=0.0, splay=0.0, betas=0.0)
    total = 0.0
    for s in range(0, N, w):
        t, o, _ = fitter_ref.fit_losses(model, P, range(s, min(N, s + w)), weights, {}, cams, 32, d["mean_b"], d["prec"],
                                        global_mask=d["gmask"], rotation_mask=d["rmask"])
        assert sorted(o) == sorted(objs)
        for k, v in o.items():
            objs[k] += v.item()
        total = total + t
    tj, tg, tt = fitter_ref.temporal(P, w_temp, d["gmask"], d["rmask"])
    (total + tj + tg + tt).backward()
    grads = dict(grot=P["global_rotation"].grad, jrot=P["joint_rotations"].grad, trans=P["trans"].grad, betas=P["betas"].grad)
    return objs, (tj.item(), tg.item(), tt.item()), grads


@pytest.mark.parametrize("key,N,window", [("synthetic", 7, 3), ("synthetic", 7, 0), ("synthetic", 5, 1), ("mouse", 11, 10), ("stick", 4, 9)])
def test_priors_match_oracle(key, N, window, tables):
    t = tables(key)
    J, nB = t.parents.shape[0], t.shapedirs.shape[0]
    d = _seeded(N, J, nB, 100 + N + J)
    weights, w_temp = [0.0, 0.0, 1.5, 2.0, 100.0, 0.1], 30.0
    r = _ref(d, weights, w_temp, window)
    objs, temp, grads = _oracle_priors(oracle_model(t), d, weights, w_temp, window)
    np.testing.assert_allclose([objs[k] for k in ("limit", "pose", "splay", "betas")], r["objs"][1:5].numpy(), rtol=F32_RTOL)
    np.testing.assert_allclose(temp, r["objs"][6:9].numpy(), rtol=F32_RTOL)
    for name, got in (("grot", r["d_pose"][:, 0]), ("jrot", r["d_pose"][:, 1:]), ("trans", r["d_trans"]), ("betas", r["d_betas"])):
        want = grads[name].numpy()
        np.testing.assert_allclose(want, got.numpy(), rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=name)


@pytest.mark.parametrize("key", ["stick", "mouse"])
def test_terms_match_reference_goldens(key, golden, tables):
    """The term values of the real reference's ``SMALFitter.forward`` / ``get_temporal`` (one window of three frames)."""
    g = golden(f"fitter_{key}")
    grot, jrot, trans = (torch.from_numpy(g[f"param_{n}"]) for n in ("global_rotation", "joint_rotations", "trans"))
    N, J = grot.shape[0], jrot.shape[1] + 1
    pose = torch.cat([grot[:, None], jrot], 1)
    r = fit_ref.priors_and_temporal(pose, trans, g["param_betas"], g["mean_betas"], g["betas_prec"], torch.ones(J, 3), g["weights"], 100.0,
                                    LIMIT, 0)
    for slot, k in ((1, "limit"), (2, "pose"), (3, "splay"), (4, "betas")):
        np.testing.assert_allclose(r["objs"][slot].item(), float(g[f"obj_{k}"]), rtol=F32_RTOL, err_msg=k)
    np.testing.assert_allclose(r["objs"][[6, 7, 8]].numpy(), g["temporal"], rtol=F32_RTOL)
    # the joint term from the oracle's projection of the same parameters
    m = oracle_model(tables(key))
    params = {n: torch.from_numpy(g[f"param_{n}"]) for n in ("betas", "log_beta_scales", "betas_trans", "global_rotation", "trans",
                                                                "joint_rotations", "fov")}
    targets = dict(sil=torch.from_numpy(g["sil_target"]), joints=torch.from_numpy(g["target_joints"]), visibility=torch.from_numpy(g["visibility"]))
    w = list(g["weights"])
    w[1] = 0.0  # no rendering needed
    _, objs, extra = fitter_ref.fit_losses(m, params, range(N), w, targets, dict(R=torch.from_numpy(g["R"]), T=torch.from_numpy(g["T"])),
                                           int(g["S"]), torch.from_numpy(g["mean_betas"]), torch.from_numpy(g["betas_prec"]))
    obj, d_proj, _ = fit_ref.joint_term(extra["proj"], targets["joints"], targets["visibility"], w[0], 1, 0)
    np.testing.assert_allclose(obj.item(), objs["joint"].item(), rtol=F32_RTOL)
    np.testing.assert_allclose(obj.item(), float(g["obj_joint"]), rtol=1e-4)  # (through the oracle's float32 LBS and projection)


@pytest.mark.parametrize("views,canon", [(1, None), (3, [4, 0, 7, 2]), (2, "first")])
def test_joint_term_matches_oracle_formula(views, canon):
    N, J, W, S = 7, 9, 3, 64
    g = torch.Generator().manual_seed(5)
    Jc = J if canon is None else 4
    sel = list(range(Jc)) if canon in (None, "first") else canon
    proj = (torch.rand(N * views, J, 2, generator=g) * S).requires_grad_()
    tgt = torch.rand(N * views, Jc, 2, generator=g) * S
    vis = torch.rand(N * views, Jc, generator=g) > 0.3
    ref = 0.0
    for s in range(0, N, W):
        idx = [f * views + v for f in range(s, min(N, s + W)) for v in range(views)]
        pj = proj[idx][:, sel]
        rj = torch.where(vis[idx][:, :, None], pj, torch.full_like(pj, -1.0))
        tj = torch.where(vis[idx][:, :, None], tgt[idx], torch.full_like(pj, -1.0))
        ref = ref + 25.0 * torch.mean((rj - tj) ** 2)  # invisible entries count in the denominator
    ref.backward()
    obj, d_proj, _ = fit_ref.joint_term(proj, tgt, vis, 25.0, views, W, None if canon in (None, "first") else canon)
    np.testing.assert_allclose(ref.item(), obj.item(), rtol=F32_RTOL)
    np.testing.assert_allclose(proj.grad.numpy(), d_proj.numpy(), rtol=1e-5, atol=0)
    unselected = [j for j in range(J) if j not in sel]
    assert not d_proj[:, unselected].any()


def test_adam_matches_torch_float64():
    g = torch.Generator().manual_seed(3)
    n, steps, lr = 1000, 60, 5e-3
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 33.0 - 30.0)
    mag[::7] = 0.0
    grads = [mag * torch.randn(n, generator=g, dtype=torch.float64) for _ in range(steps)]
    pt = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pt], lr=lr, betas=(0.5, 0.999), eps=1e-8, foreach=False)
    for k, (p, m, v) in enumerate(fit_ref.adam(p0, grads, lr)):
        pt.grad = grads[k].clone()
        opt.step()
        st = opt.state[pt]
        np.testing.assert_allclose(p.numpy(), pt.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m.numpy(), st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v.numpy(), st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert torch.equal(p[::7], p0[::7]) and not m[::7].any() and not v[::7].any()
    # a continued run with the moments carried is the same run
    half = fit_ref.adam(p0, grads[:30], lr)[-1]
    rest = fit_ref.adam(half[0], grads[30:], lr, exp_avg=half[1], exp_avg_sq=half[2], step0=30)[-1]
    for a, b in zip(rest, (p, m, v)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("window", [3, 0, 1, 10])
def test_sharded_sum_equals_unsharded(window):
    """Three shards with halos, one of a single frame, add up to the unsharded evaluation (objectives, shape-prior gradient)
    and reproduce its per-frame gradients."""
    N, J, nB = 7, 9, 3
    d = _seeded(N, J, nB, 21)
    weights, w_temp = [25.0, 0.0, 1.5, 2.0, 100.0, 0.1], 30.0
    full = _ref(d, weights, w_temp, window)
    rows = torch.cat([d["grot"], d["jrot"].reshape(N, -1), d["trans"]], 1)
    objs, d_betas, dp, dt = 0.0, 0.0, [], []
    for f0, n in ((0, 3), (3, 1), (4, 3)):
        part = {k: (v[f0:f0 + n] if k in ("grot", "jrot", "trans") else v) for k, v in d.items()}
        r = _ref(part, weights, w_temp, window, frame0=f0, N_total=N, halo_prev=rows[f0 - 1] if f0 > 0 else None,
                 halo_next=rows[f0 + n] if f0 + n < N else None)
        objs, d_betas = objs + r["objs"], d_betas + r["d_betas"]
        dp.append(r["d_pose"])
        dt.append(r["d_trans"])
    np.testing.assert_allclose(objs.numpy(), full["objs"].numpy(), rtol=1e-13)
    np.testing.assert_allclose(d_betas.numpy(), full["d_betas"].numpy(), rtol=1e-13)
    np.testing.assert_allclose(torch.cat(dp).numpy(), full["d_pose"].numpy(), rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(torch.cat(dt).numpy(), full["d_trans"].numpy(), rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("window", [3, 0, 1, 10])
def test_window_table_sums_to_objectives(window):
    N, J, nB, views = 7, 9, 3, 2
    d = _seeded(N, J, nB, 22)
    g = torch.Generator().manual_seed(23)
    weights = [25.0, 500.0, 1.5, 2.0, 100.0, 0.1]
    proj, tgt = torch.rand(N * views, J, 2, generator=g) * 64, torch.rand(N * views, 5, 2, generator=g) * 64
    vis, canon = torch.rand(N * views, 5, generator=g) > 0.3, [8, 1, 3, 0, 6]
    loss_img = torch.rand(N * views, generator=g) * 100
    ps = fit_ref.pix_scale(N, views, 64, weights[1], window)
    pose, mask = torch.cat([d["grot"][:, None], d["jrot"]], 1), torch.cat([d["gmask"], d["rmask"]], 0)
    tab = fit_ref.window_terms(pose, mask, d["betas"], d["mean_b"], d["prec"], weights, LIMIT, window, proj=proj, target=tgt, visibility=vis,
                               views=views, canon=canon, loss_img=loss_img, pix_scale=ps)
    w = window if window > 0 else N
    assert tab.shape == ((N + w - 1) // w, 6)
    full = _ref(d, weights, 0.0, window)["objs"].clone()
    full[0] = fit_ref.joint_term(proj, tgt, vis, weights[0], views, window, canon)[0]
    full[5] = (loss_img.double() * ps).sum()
    np.testing.assert_allclose(tab.sum(0).numpy(), full[:6].numpy(), rtol=1e-13)
    with pytest.raises(ValueError):
        fit_ref.window_terms(pose[2:], mask, d["betas"], d["mean_b"], d["prec"], weights, LIMIT, 3, frame0=2, N_total=N)


def test_hinge_gradient_at_the_tie():
    """A joint rotation exactly on +-limit gets +-half the per-element scale, as autograd of torch.max(x - lim, 0) gives."""
    N, J, W, w_limit = 4, 3, 3, 100.0
    pose = torch.zeros(N, J, 3)
    pose[:, 1, 0], pose[:, 1, 1], pose[:, 2, 0], pose[:, 2, 1] = LIMIT, -LIMIT, 0.02, -0.02
    r = fit_ref.priors_and_temporal(pose, torch.zeros(N, 3), None, None, None, torch.ones(J, 3), [0, 0, 0, 0, w_limit, 0], 0.0, LIMIT, W)
    scale = w_limit / (fit_ref.window_sizes(N, W) * (3 * J - 3))  # frames 0..2 in a window of 3, frame 3 alone
    np.testing.assert_allclose(scale.numpy(), [w_limit / 18, w_limit / 18, w_limit / 18, w_limit / 6], rtol=1e-15)
    g = r["d_pose"]
    for col, want in ((g[:, 1, 0], 0.5 * scale), (g[:, 1, 1], -0.5 * scale), (g[:, 2, 0], scale), (g[:, 2, 1], -scale)):
        np.testing.assert_allclose(col.numpy(), want.numpy(), rtol=1e-15)
    assert not g[:, 0].any() and not g[:, :, 2].any()
    # the float32 oracle uses the same torch call and agrees
    x = torch.tensor([0.01, -0.01], requires_grad=True)
    z = torch.zeros_like(x)
    (torch.max(x - 0.01, z) + torch.max(-0.01 - x, z)).sum().backward()
    assert x.grad.tolist() == [0.5, -0.5]
