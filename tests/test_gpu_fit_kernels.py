"""The loss and optimiser kernels of ``smilify_amd/csrc/fit.hip`` against the float64 reference ``tests/fit_ref.py``, entry point
by entry point, at the shapes where their grid-stride loops stride, at partial windows, shards with halos, every config flag,
and on the kink of the joint-limit hinge.

Bounds (none is taken from the kernels):

* exact 0: frozen / masked gradient rows, ``d_proj`` of unselected joints, objectives of all-zero inputs, parameters and moments
  of zero-gradient Adam elements (the per-element bound below is 0 there, so the same assertion covers them);
* per-element gradients: ``|got - ref| <= 16 * 2^-24 * sum|contribution|`` (at most 6 rounded operations per contribution and
  5 additions; no fast-math), the absolute sum from ``fit_ref``;
* ``d_betas``: forward bound of a length-nB dot product applied twice, ``gamma(2 nB + 5) * scale * |P| (|diff| |P|)`` with
  ``gamma(n) = n u / (1 - n u)``, ``u = 2^-24`` (nB + 1 roundings per inner product incl. the subtraction, 3 for the scaling);
* reduced objectives: ``rtol = 2e-5`` for every launch below its grid cap and every launch with one workgroup per output, the
  README's ``1e-4`` only at full size, past the cap (4096 x 35 priors, 82 944 / 101 376 joint items, 147 456 images); sums of
  signed terms (fov) are measured against the sum of absolute values;
* Adam: the error against float64 of parameter and both moments, max-abs and RMS, at most 4 x that of ``torch.optim.Adam`` in
  float32 on the CPU over the same gradient sequence (recomputed here).  For tensors of fewer than 64 elements only, the
  yardstick is floored at ``2^-24 * max|value|`` (half an ulp, what storing a float32 result costs): on a one-element tensor
  the CPU's own error can be 0 by chance, which says nothing about the kernel.

Measured on an MI355X (worst case over the module): worst relative error of a reduced objective 9.1e-7 (smil_prior_losses, 4096 x 35,
512 workgroups of float atomics, whose order varies from run to run; 7.8e-7 in smil_fit_epilogue), 1.7e-7 at single-workgroup shapes,
2.6e-7 smil_joint_loss (82 944 items), 1.6e-7 smil_window_terms, 1.5e-7 the silhouette objective (147 456 images), 9.0e-8
smil_image_abs_sum - nothing near 2e-5, the 512-long chain of atomics included.  Per-element gradients reach 0.26 of their bound
(d_pose), 0.16 (d_trans), 0.11 (d_proj), d_betas 0.28 of its; the fov reduction 0.013 of its, and equals smil_fov_reduce bit for bit.
Adam, kernel error / float32-CPU error against float64 (max-abs or RMS, worst over all lengths and step counts): parameter 2.55,
exp_avg 2.57, exp_avg_sq 3.09, all at 255 / 256 elements where a few elements with gradients near 1e3 decide both errors (1.57, 1.50,
1.03 at 131 073 and 600 001 elements).  With ``1 - beta2`` formed as ``1.0f - 0.999f`` (1.3e-5 relative bias), as the
kernels did before, exp_avg_sq is 53 .. 736 x the yardstick over steps 1 .. 10 and 6 .. 11 x after 200 steps.
smil_adam_step_multi equals smil_adam_step bit for bit.
"""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

import fit_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
LIMIT = float(np.float32(0.01))
WEIGHTS = (25.0, 500.0, 1.5, 2.0, 100.0, 0.1)  # w_j2d, w_reproj, w_betas, w_pose, w_limit, w_splay
W_TEMP = 30.0
ENTRIES = ("prior_losses", "fit_epilogue")


def _engine():
    from smilify_amd import engine

    return engine


PRIOR_CAP, JOINT_CAP, SIL_CAP = 512 * 256, 256 * 256, 64 * 256  # work items at which a launch reaches its grid cap


def _rtol(work_items=0, cap_items=None):
    """Ceiling of a reduced objective: 2e-5, what the single-workgroup test asserts, for every launch below its grid cap and for
    every launch that gives each output a workgroup of its own (window terms, image sums, fov: no chain of atomics at any size);
    the README's 1e-4 only at full size, where the work exceeds ``cap_items`` = cap x 256, every workgroup strides and the
    chain of float atomics has its full length."""
    return 1e-4 if cap_items is not None and work_items > cap_items else 2e-5


def _cu(x, dtype=torch.float32):
    return None if x is None else x.detach().to(device=DEV, dtype=dtype).contiguous()


def _report(name, **figures):
    print(f"[fit-kernels] {name}: " + "  ".join(f"{k}={v:.3e}" for k, v in figures.items()))


def _check_objective(got, ref, rtol, what):
    """|got - ref| <= rtol |ref| for every slot, which asks exactly 0 where the reference is 0.  Returns the worst relative error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    rel = np.where(ref != 0, err / np.where(ref != 0, np.abs(ref), 1.0), np.where(err == 0, 0.0, np.inf))
    assert (err <= rtol * np.abs(ref)).all(), f"{what}: got {got} want {ref} (relative error {rel}, bound {rtol})"
    return float(rel.max()) if rel.size else 0.0


def _check_elements(got, ref, bound, what):
    """Every element within its own bound (a bound of 0 asks for the exact value).  Returns the worst error / bound."""
    got, ref, bound = got.detach().cpu().double(), ref.double(), bound.double()
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        k = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at flat index {k}: got "
                             f"{got.reshape(-1)[k].item()!r} want {ref.reshape(-1)[k].item()!r} bound {bound.reshape(-1)[k].item()!r}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# prior losses / epilogue
# ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    N_total: int
    J: int
    window: int
    frame0: int = 0
    N: Optional[int] = None            # shard length (None: the whole sequence)
    nB: int = 3
    weights: Tuple[float, ...] = WEIGHTS
    w_temp: float = W_TEMP
    train: Tuple[bool, bool, bool] = (True, True, True)
    accumulate: bool = False
    zero_mask_row: bool = False
    values: str = "random"             # random | zero | sides | kink
    halos: bool = True                 # False: pass no halo rows (only legal with w_temp = 0)
    seed: int = 0

    @property
    def n(self):
        return self.N_total - self.frame0 if self.N is None else self.N


def _inputs(c: Case):
    """float32 CPU inputs of the shard [frame0, frame0 + n) cut from a seeded sequence of N_total frames."""
    g = torch.Generator().manual_seed(1000 + c.seed + 7 * c.N_total + 13 * c.J + 31 * c.window)
    Nt, J, nB = c.N_total, c.J, c.nB
    grot = 0.5 * torch.randn(Nt, 3, generator=g)
    trans = 0.2 * torch.randn(Nt, 3, generator=g)
    lim32 = torch.tensor(LIMIT)
    if c.values == "random":
        jrot = 0.02 * torch.randn(Nt, J - 1, 3, generator=g)
    elif c.values == "sides":  # within 1 % of +-limit on either side; the inner ones lie in [0.99 limit, limit)
        f = 0.9901 + 0.0198 * torch.rand(Nt, J - 1, 3, generator=g)
        jrot = lim32 * f * torch.where(torch.rand(Nt, J - 1, 3, generator=g) < 0.5, -1.0, 1.0)
        inner = jrot.abs() < lim32
        assert (jrot.abs()[inner] >= 0.99 * LIMIT).all() and inner.any() and (~inner).any()
    elif c.values == "kink":  # most values EXACTLY on +-limit, the rest clearly inside / outside
        pick = torch.randint(0, 6, (Nt, J - 1, 3), generator=g)
        jrot = torch.tensor([LIMIT, -LIMIT, LIMIT, -LIMIT, 0.02, -0.004])[pick]
        assert (jrot == lim32).any() and (jrot == -lim32).any()
    else:  # the reference's starting point: no joint rotation, one global rotation for all frames, betas on their mean
        jrot = torch.zeros(Nt, J - 1, 3)
        grot = torch.tensor([-1.2092, -1.2092, -1.2092]).repeat(Nt, 1)
        trans = torch.zeros(Nt, 3)
    mask = torch.cat([torch.tensor([[1.0, 0.0, 1.0]]), (torch.rand(J - 1, 3, generator=g) > 0.2).float()], 0)
    if c.values in ("kink", "sides"):
        mask[1:] = 1.0
    elif J > 2:
        mask[J - 1, 0] = 0.5  # a non-binary entry: the mask scales the value AND the gradient
    if c.zero_mask_row:
        mask[J // 2 if J > 2 else 1] = 0.0
    A = torch.randn(nB, nB, generator=g)
    prec = torch.tril(A) + 2.0 * torch.eye(nB)  # lower triangular, not symmetric: diff @ prec != prec @ diff
    mean_b = 0.1 * torch.randn(nB, generator=g)
    betas = mean_b.clone() if c.values == "zero" else torch.randn(nB, generator=g)
    pose = torch.cat([grot[:, None], jrot], 1)
    rows = torch.cat([pose.reshape(Nt, -1), trans], 1)
    f0, n = c.frame0, c.n
    up = None
    if c.accumulate:
        up = (torch.randn(n, J, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(nB, generator=g))
    return dict(pose=pose[f0:f0 + n].contiguous(), trans=trans[f0:f0 + n].contiguous(), betas=betas, mean_b=mean_b, prec=prec, mask=mask,
                halo_prev=rows[f0 - 1] if (c.halos and f0 > 0) else None,
                halo_next=rows[f0 + n] if (c.halos and f0 + n < Nt) else None, upstream=up)


def _reference(c: Case, inp):
    return fit_ref.priors_and_temporal(inp["pose"], inp["trans"], inp["betas"], inp["mean_b"], inp["prec"], inp["mask"], c.weights, c.w_temp,
                                       LIMIT, c.window, c.frame0, c.N_total, inp["halo_prev"], inp["halo_next"], c.train,
                                       None if inp["upstream"] is None else inp["upstream"][:2])


def _config(c: Case):
    return _engine().fit_config(c.n, c.J, c.nB, c.window, c.weights, c.w_temp, frame0=c.frame0, N_total=c.N_total, limit=0.01,
                                train_global=c.train[0], train_joints=c.train[1], train_trans=c.train[2])


def _sil_and_fov_inputs(n_img, nfov_kind, seed=0, views=3):
    g = torch.Generator().manual_seed(77 + seed + n_img)
    loss_img = 100.0 * torch.rand(n_img, generator=g)
    scale = 1e-4 * (0.5 + torch.rand(n_img, generator=g))
    M = views * n_img
    nfov = {"one": 1, "views": views, "N": M}[nfov_kind]
    return loss_img, scale, torch.randn(M, generator=g), 30.0 + 60.0 * torch.rand(nfov, generator=g), views


def _cameras(fov, views):
    eng = _engine()
    return eng.CameraSet(R=torch.eye(3, device=DEV)[None].contiguous(), T=torch.zeros(1, 3, device=DEV), fov=_cu(fov), aspect=None, views=views, S=64)


def _launch(entry, c: Case, inp, sil=None):
    """Run one entry point; returns objs (10,), d_pose, d_trans, d_betas (and d_fov for the epilogue), all on the CPU."""
    eng = _engine()
    n, J, nB = c.n, c.J, c.nB
    objs = torch.zeros(10, device=DEV)
    if c.accumulate:
        dp, dt, db = (_cu(t).clone() for t in inp["upstream"])
    else:  # stale contents must be overwritten, not added to
        dp, dt, db = torch.full((n, J, 3), 7.0, device=DEV), torch.full((n, 3), -7.0, device=DEV), torch.zeros(nB, device=DEV)
    args = (_config(c), _cu(inp["pose"]), _cu(inp["trans"]), _cu(inp["betas"]), _cu(inp["mean_b"]), _cu(inp["prec"]), _cu(inp["mask"]), objs,
            dp, dt, db)
    kw = dict(halo_prev=_cu(inp["halo_prev"]), halo_next=_cu(inp["halo_next"]), accumulate=c.accumulate)
    d_fov = None
    if entry == "prior_losses":
        eng.prior_losses(*args, **kw)
    else:
        loss_img, scale, d_fov_img, fov, views = sil
        cams = _cameras(fov, views)
        d_fov = torch.full((fov.numel(),), 7.0, device=DEV)
        eng.fit_epilogue(*args, **kw, loss_img=_cu(loss_img), pix_scale=_cu(scale), cams=cams, d_fov_img=_cu(d_fov_img), d_fov=d_fov)
        d_fov = (d_fov.cpu(), eng.fov_reduce(cams, _cu(d_fov_img)).cpu())
    torch.cuda.synchronize()
    return objs.cpu(), dp.cpu(), dt.cpu(), db.cpu(), d_fov


def _check_sil_and_fov(objs5, d_fov, sil, name):
    loss_img, scale, d_fov_img, fov, views = sil
    want = (loss_img.double() * scale.double()).sum().item()
    rel = _check_objective([objs5], [want], _rtol(loss_img.numel(), SIL_CAP), f"{name} objs[5]")
    got, alone = d_fov
    assert torch.equal(got, alone), f"{name}: the epilogue's fov reduction differs from smil_fov_reduce on the same input"
    ref, ref_abs = fit_ref.fov_reduce(d_fov_img, fov)
    r = _check_elements(got, ref, _rtol() * ref_abs, f"{name} d_fov")
    _report(name, sil_rel=rel, fov_err_over_bound=r, fov_rtol=_rtol())


def _run_and_check(entry, c: Case, name, sil_kind=(257, "views")):
    inp = _inputs(c)
    ref = _reference(c, inp)
    sil = _sil_and_fov_inputs(*sil_kind, seed=c.seed) if entry == "fit_epilogue" else None
    objs, dp, dt, db, d_fov = _launch(entry, c, inp, sil)
    work = c.n * (3 * c.J + 3)
    want = ref["objs"].numpy().copy()
    slots = [1, 2, 3, 6, 7, 8]
    rel = _check_objective(objs.numpy()[slots], want[slots], _rtol(work, PRIOR_CAP), f"{name} objs{slots}")
    rel_b = _check_objective(objs.numpy()[[4]], want[[4]], 2e-5, f"{name} objs[4]")  # one thread, nB terms
    assert objs[0] == 0 and objs[9] == 0 and (entry == "fit_epilogue" or objs[5] == 0), f"{name}: a slot this entry does not own was written"
    if c.values == "zero":
        assert not objs[[0, 1, 2, 3, 4, 6, 7, 8, 9]].any(), f"{name}: {objs}"
    r_pose = _check_elements(dp, ref["d_pose"], 16 * U * ref["abs_pose"], f"{name} d_pose")
    r_trans = _check_elements(dt, ref["d_trans"], 16 * U * ref["abs_trans"], f"{name} d_trans")
    # frozen and fully masked rows (bound 0 above); spelled out
    for flag, block in zip(c.train, (dp[:, 0], dp[:, 1:], dt)):
        assert flag or not block.any(), f"{name}: a frozen block has a gradient"
    assert not dp[:, inp["mask"] == 0].any(), f"{name}: a masked entry has a gradient"
    nu = (2 * c.nB + 5) * U
    want_b, bound_b = ref["d_betas"], nu / (1 - nu) * ref["abs_betas"]
    if c.accumulate:  # the shape prior's gradient is always added to what the buffer holds
        want_b = want_b + inp["upstream"][2].double()
        bound_b = bound_b + U * want_b.abs()  # the atomic add's own rounding
    r_betas = _check_elements(db, want_b, bound_b, f"{name} d_betas")
    if sil is not None:
        _check_sil_and_fov(objs[5].item(), d_fov, sil, name)
    _report(name, obj_rel=rel, obj_rtol=_rtol(work, PRIOR_CAP), betas_obj_rel=rel_b, d_pose=r_pose, d_trans=r_trans, d_betas=r_betas)
    return inp, objs


SHAPE_CASES = {f"N{N}-J{J}-w{w if w < 10 ** 6 else 'big'}": Case(N, J, w if w < 10 ** 6 else N + 5)
               for N in (1, 2, 7, 4096) for J in (2, 9, 35) for w in (0, 1, 3, 10, 10 ** 6)}
BASE = Case(7, 9, 3)
_ONLY = {"betas": 2, "pose": 3, "limit": 4, "splay": 5}
FLAG_CASES = {
    # shards of a 7- and an 11-frame sequence: frame0 > 0, each halo present / absent, one frame with both halos
    "shard-tail-prev-halo": replace(BASE, frame0=3),
    "shard-head-next-halo": replace(BASE, N=3),
    "shard-one-frame-both-halos": replace(BASE, frame0=3, N=1),
    "shard-inside-window-both-halos": replace(BASE, frame0=2, N=3),
    "shard-partial-last-window": Case(11, 9, 4, frame0=8),
    "shard-middle-two-windows": Case(11, 35, 3, frame0=3, N=6, nB=20),
    "shard-no-halos-w_temp0": replace(BASE, frame0=2, N=3, w_temp=0.0, halos=False),
    "shard-window0": replace(BASE, window=0, frame0=3, N=2),
    "train-global-off": replace(BASE, train=(False, True, True)),
    "train-joints-off": replace(BASE, train=(True, False, True)),
    "train-trans-off": replace(BASE, train=(True, True, False)),
    "accumulate": replace(BASE, accumulate=True),
    "accumulate-frozen-joints": replace(BASE, accumulate=True, train=(True, False, True)),
    "accumulate-4096x35": Case(4096, 35, 10, accumulate=True),
    "zero-mask-row": replace(BASE, zero_mask_row=True),
    **{f"only-w_{k}": replace(BASE, weights=tuple(WEIGHTS[i] if i == pos else 0.0 for i in range(6)), w_temp=0.0) for k, pos in _ONLY.items()},
    "only-w_temp": replace(BASE, weights=(0.0,) * 6),
    "nB1": replace(BASE, nB=1),
    "nB20": replace(BASE, nB=20),
    "nB64": replace(BASE, nB=64),
    "nB64-shard": replace(BASE, nB=64, frame0=3),
    "zero-init": replace(BASE, values="zero"),
    "zero-init-4096x35": Case(4096, 35, 10, values="zero"),
    "both-sides-of-limit": replace(BASE, values="sides"),
    "both-sides-of-limit-4096x35": Case(4096, 35, 10, values="sides"),
    "on-the-kink": replace(BASE, values="kink"),
    "on-the-kink-partial-window": Case(11, 35, 4, values="kink"),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(SHAPE_CASES))
def test_priors_shapes(name, entry):
    _run_and_check(entry, SHAPE_CASES[name], f"{entry}[{name}]")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(FLAG_CASES))
def test_priors_flags_shards_values(name, entry):
    _run_and_check(entry, FLAG_CASES[name], f"{entry}[{name}]")


@pytest.mark.parametrize("entry", ENTRIES)
def test_kink_gradient_is_half_the_scale(entry):
    """Spelled out without the reference: on +-limit the limit term's gradient is +-w_limit / (2 b_w 3(J-1))."""
    eng = _engine()
    N, J, W, w_limit = 4, 3, 3, 100.0
    pose = torch.zeros(N, J, 3)
    pose[:, 1, 0], pose[:, 1, 1], pose[:, 2, 0], pose[:, 2, 1] = LIMIT, -LIMIT, 0.02, -0.02
    c = Case(N, J, W, nB=1, weights=(0, 0, 0, 0, w_limit, 0), w_temp=0.0)
    inp = dict(_inputs(c), pose=pose, mask=torch.ones(J, 3))
    sil = _sil_and_fov_inputs(1, "one") if entry == "fit_epilogue" else None
    _, dp, dt, _, _ = _launch(entry, c, inp, sil)
    scale = torch.tensor([w_limit / 18, w_limit / 18, w_limit / 18, w_limit / 6])  # frames 0..2 share a window, frame 3 is alone
    for col, want in ((dp[:, 1, 0], 0.5 * scale), (dp[:, 1, 1], -0.5 * scale), (dp[:, 2, 0], scale), (dp[:, 2, 1], -scale)):
        np.testing.assert_allclose(col.numpy(), want.numpy(), rtol=4 * U, atol=0)
    assert not dp[:, 0].any() and not dp[:, :, 2].any() and not dt.any()


@pytest.mark.parametrize("entry", ENTRIES)
def test_too_many_betas_is_refused(entry):
    from smilify_amd import _lib

    c = replace(BASE, nB=65)
    inp = _inputs(c)
    with pytest.raises(_lib.SmilError) as e:
        _launch(entry, c, inp, _sil_and_fov_inputs(1, "one") if entry == "fit_epilogue" else None)
    assert "nB too large" in str(e.value) and "code" in str(e.value)
    assert b"nB too large" in _lib.load().smil_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("nfov", ["one", "views", "N"])
@pytest.mark.parametrize("n_img", [1, 255, 256, 257, 147456])
def test_epilogue_silhouette_and_fov(n_img, nfov):
    _run_and_check("fit_epilogue", BASE, f"fit_epilogue[n_img={n_img}-nFov={nfov}]", sil_kind=(n_img, nfov))


# ------------------------------------------------------------------------------------------------------------------------
# 2-D joint loss
# ------------------------------------------------------------------------------------------------------------------------
def _joint_inputs(N, J, views, canon_kind, vis_kind, seed=0, S=64):
    g = torch.Generator().manual_seed(500 + seed + N + views)
    if canon_kind == "all":
        Jc, canon = J, None
    elif canon_kind == "first":
        Jc, canon = max(1, J - 2), None
    else:
        Jc = max(1, J - 2)
        canon = torch.randperm(J, generator=g)[:Jc].tolist()
    proj = S * torch.rand(N * views, J, 2, generator=g)
    tgt = S * torch.rand(N * views, Jc, 2, generator=g)
    vis = dict(off=torch.zeros(N * views, Jc), on=torch.ones(N * views, Jc), random=(torch.rand(N * views, Jc, generator=g) > 0.3).float())[vis_kind]
    return Jc, canon, proj, tgt, vis.int()


def _check_joint(c: Case, views, canon_kind, vis_kind, name):
    eng = _engine()
    Jc, canon, proj, tgt, vis = _joint_inputs(c.n, c.J, views, canon_kind, vis_kind)
    obj, d_ref, d_abs = fit_ref.joint_term(proj, tgt, vis, c.weights[0], views, c.window, canon, c.frame0, c.N_total)
    objs = torch.zeros(10, device=DEV)
    d_proj = torch.full((c.n * views, c.J, 2), 7.0, device=DEV)
    eng.joint_loss(_config(c), views, Jc, None if canon is None else _cu(torch.tensor(canon), torch.int32), _cu(proj), _cu(tgt),
                   _cu(vis, torch.int32), objs, d_proj)
    torch.cuda.synchronize()
    work = c.n * views * Jc
    rel = _check_objective(objs.cpu().numpy()[[0]], [obj.item()], _rtol(work, JOINT_CAP), f"{name} objs[0]")
    assert not objs[1:].any()
    r = _check_elements(d_proj, d_ref, 16 * U * d_abs, f"{name} d_proj")
    sel = list(range(Jc)) if canon is None else canon
    unsel = [j for j in range(c.J) if j not in sel]
    assert not d_proj[:, unsel].any(), f"{name}: d_proj of an unselected joint is not 0"
    if vis_kind == "off":
        assert not d_proj.any() and objs[0] == 0
    _report(name, obj_rel=rel, obj_rtol=_rtol(work, JOINT_CAP), d_proj=r)


@pytest.mark.parametrize("vis_kind", ["off", "on", "random"])
@pytest.mark.parametrize("canon_kind", ["all", "first", "permuted"])
@pytest.mark.parametrize("views", [1, 3, 18])
def test_joint_loss(views, canon_kind, vis_kind):
    _check_joint(BASE, views, canon_kind, vis_kind, f"joint_loss[v{views}-{canon_kind}-{vis_kind}]")


@pytest.mark.parametrize("name,c,views,canon_kind", [
    ("strided-82944-items", Case(512, 9, 10), 18, "all"),       # > 256 blocks x 256 threads
    ("strided-permuted", Case(512, 35, 0), 6, "permuted"),      # 101 376 items
    ("shard-partial-window", Case(11, 9, 4, frame0=8), 3, "permuted"),
    ("window-larger-than-sequence", Case(7, 9, 12), 3, "first"),
    ("one-frame-two-joints", Case(1, 2, 1), 1, "all"),
])
def test_joint_loss_strided_and_sharded(name, c, views, canon_kind):
    _check_joint(c, views, canon_kind, "random", f"joint_loss[{name}]")


# ------------------------------------------------------------------------------------------------------------------------
# per-window restatement
# ------------------------------------------------------------------------------------------------------------------------
WINDOW_CASES = {
    "w3-partial-last": (BASE, 2, True, True),
    "w0": (replace(BASE, window=0), 2, True, True),
    "w1": (replace(BASE, window=1), 2, True, True),
    "w-larger-than-sequence-714-items": (Case(7, 35, 12), 3, True, True),   # one window, more items than one pass of 256 threads
    "w10-4096x35": (Case(4096, 35, 10), 1, True, True),
    "w0-4096x9": (Case(4096, 9, 0), 1, True, True),
    "shard-at-later-window": (Case(11, 9, 3, frame0=6), 2, True, True),
    "shard-middle": (Case(11, 9, 3, frame0=3, N=6), 2, True, True),
    "no-proj": (BASE, 2, False, True),
    "no-loss-img": (BASE, 2, True, False),
    "kink-values": (Case(11, 35, 4, values="kink"), 1, True, True),
}


@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_window_terms(name):
    eng = _engine()
    c, views, with_proj, with_sil = WINDOW_CASES[name]
    inp = _inputs(c)
    objs_total, *_ = _launch("prior_losses", c, inp)
    Jc, canon, proj, tgt, vis = _joint_inputs(c.n, c.J, views, "permuted", "random", seed=3)
    g = torch.Generator().manual_seed(9)
    loss_img = 100.0 * torch.rand(c.n * views, generator=g)
    cfg = _config(c)
    ps = eng.pix_scale(cfg, views, 64, DEV)
    np.testing.assert_allclose(ps.cpu().numpy(), fit_ref.pix_scale(c.n, views, 64, c.weights[1], c.window, c.frame0, c.N_total).numpy(), rtol=4 * U)
    got = eng.window_terms(cfg, views, Jc, _cu(torch.tensor(canon), torch.int32), _cu(proj) if with_proj else None, _cu(tgt), _cu(vis, torch.int32),
                           _cu(inp["pose"]), _cu(inp["mask"]), _cu(objs_total), _cu(loss_img) if with_sil else None, ps).cpu().numpy()
    ref = fit_ref.window_terms(inp["pose"], inp["mask"], inp["betas"], inp["mean_b"], inp["prec"], c.weights, LIMIT, c.window, c.frame0, c.N_total,
                               proj=proj if with_proj else None, target=tgt, visibility=vis, views=views, canon=canon,
                               loss_img=loss_img if with_sil else None, pix_scale=ps.cpu()).numpy()
    assert got.shape == ref.shape
    worst = 0.0
    for k in range(ref.shape[0]):
        for slot in range(6):  # one workgroup per window, fixed order, no atomics: 2e-5 at every size
            worst = max(worst, _check_objective([got[k, slot]], [ref[k, slot]], _rtol(), f"window_terms[{name}] window {k} slot {slot}"))
    if not with_proj:
        assert not got[:, 0].any()
    if not with_sil:
        assert not got[:, 5].any()
    _report(f"window_terms[{name}]", worst_rel=worst)


def test_window_terms_refuses_a_shard_inside_a_window():
    from smilify_amd import _lib

    eng = _engine()
    c = replace(BASE, frame0=2, N=3)
    inp = _inputs(c)
    with pytest.raises(_lib.SmilError, match="starts inside a window"):
        eng.window_terms(_config(c), 1, 1, None, None, None, None, _cu(inp["pose"]), _cu(inp["mask"]), torch.zeros(10, device=DEV), None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# pix_scale, silhouette objective, mask_rows, image_abs_sum
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 100, 512])
@pytest.mark.parametrize("c", [BASE, replace(BASE, window=0), Case(11, 9, 4, frame0=8), Case(300, 2, 7)], ids=["w3", "w0", "shard", "300-frames"])
def test_pix_scale(c, S):
    eng = _engine()
    views, w = 3, np.float32(c.weights[1])
    got = eng.pix_scale(_config(c), views, S, DEV).cpu().numpy()
    bw = fit_ref.window_sizes(c.n, c.window, c.frame0, c.N_total).repeat_interleave(views).numpy().astype(np.float32)
    want = w / (bw * np.float32(views) * np.float32(S) * np.float32(S))  # the kernel's own formula, evaluated in float32
    assert want.dtype == np.float32 and got.shape == want.shape
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()
    np.testing.assert_allclose(got, fit_ref.pix_scale(c.n, views, S, c.weights[1], c.window, c.frame0, c.N_total).numpy(), rtol=8 * U)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 147456])
def test_sil_objective(n):
    eng = _engine()
    loss_img, scale, *_ = _sil_and_fov_inputs(n, "one")
    objs = torch.zeros(10, device=DEV)
    eng.sil_objective(_cu(loss_img), _cu(scale), objs)
    want = (loss_img.double() * scale.double()).sum().item()
    rel = _check_objective([objs[5].item()], [want], _rtol(n, SIL_CAP), f"sil_objective[{n}]")
    assert not objs[[0, 1, 2, 3, 4, 6, 7, 8, 9]].any()
    eng.sil_objective(_cu(loss_img), _cu(scale), objs)  # the slot accumulates
    _check_objective([objs[5].item()], [2 * want], _rtol(n, SIL_CAP), f"sil_objective[{n}] twice")
    _report(f"sil_objective[{n}]", rel=rel, rtol=_rtol(n, SIL_CAP))


@pytest.mark.parametrize("rows,cols", [(1, 3), (7, 27), (300, 1), (5000, 108)])  # 540 000 elements: beyond 2048 x 256
def test_mask_rows(rows, cols):
    eng = _engine()
    g = torch.Generator().manual_seed(rows)
    x, m = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
    m[::3] = 0.0
    got = eng.mask_rows(_cu(x), _cu(m)).cpu()
    assert torch.equal(got, (x.double() * m.double()).float())  # one rounding: the float32 product is the rounded exact one


@pytest.mark.parametrize("dtype", ["float", "uint8"])
@pytest.mark.parametrize("pixels", [1, 255, 257, 100 * 100, 512 * 512])
def test_image_abs_sum(pixels, dtype):
    eng = _engine()
    g = torch.Generator().manual_seed(pixels)
    n = 3
    img = torch.randn(n, pixels, generator=g) if dtype == "float" else torch.randint(0, 256, (n, pixels), generator=g, dtype=torch.uint8)
    got = eng.image_abs_sum(img.to(DEV).contiguous()).cpu().numpy()
    want = img.double().abs().sum(1).numpy()
    rel = _check_objective(got, want, _rtol(), f"image_abs_sum[{pixels}-{dtype}]")
    _report(f"image_abs_sum[{pixels}-{dtype}]", rel=rel, rtol=_rtol())


@pytest.mark.parametrize("dtype", ["float", "uint8"])
def test_image_abs_sum_beyond_2_pow_24(dtype):
    """A 512^2 image of 255s sums to 255 * 2^18 > 2^24.  With 256 threads striding the image, every thread's running sum is 255 * m,
    m <= 2^10, and every sum of whole threads' totals is 255 * 2^10 * k, k <= 2^8: at most 18 significant bits, so no addition
    rounds in any order of the tree, and the result is exact.  The second image is 255 on its first half only."""
    eng = _engine()
    img = torch.full((2, 512, 512), 255, dtype=torch.uint8)
    img[1, 256:] = 0
    img = img.float() if dtype == "float" else img
    got = eng.image_abs_sum(img.to(DEV).contiguous()).cpu().double().tolist()
    assert got == [255.0 * 2 ** 18, 255.0 * 2 ** 17]


# ------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 5e-3, 0.5, 0.999, 1e-8


def _adam_problem(n, seed=0):
    g = torch.Generator().manual_seed(4000 + seed + n)
    p0 = torch.randn(n, generator=g)
    mag = 10.0 ** (33.0 * torch.rand(n, generator=g, dtype=torch.float64) - 30.0)  # 1e-30 .. 1e3
    mag[3::7] = 0.0  # these elements never receive a gradient

    def grads(steps):
        for _ in range(steps):
            yield (mag * torch.randn(n, generator=g, dtype=torch.float64)).float()

    return p0, mag == 0, grads


class _Torch32:
    """The yardstick: torch.optim.Adam in float32 on the CPU (single-tensor form)."""

    def __init__(self, p0, lr, m0=None, v0=None, step0=0):
        self.p = p0.clone().requires_grad_()
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=(B1, B2), eps=EPS, foreach=False)
        if step0:
            self.opt.state[self.p] = dict(step=torch.tensor(float(step0)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())

    def step(self, g):
        self.p.grad = g.clone()
        self.opt.step()

    def state(self):
        st = self.opt.state[self.p]
        return self.p.detach(), st["exp_avg"], st["exp_avg_sq"]


def _errors(state, ref):
    out = []
    for got, want in zip(state, ref):
        e = (got.detach().cpu().double() - want).abs()
        out.append((e.max().item(), e.pow(2).mean().sqrt().item()))
    return out


def _check_adam(name, kernel_state, yard_state, ref, factor=4.0):
    worst = 0.0
    floor = [U * r.abs().max().item() if ref[0].numel() < 64 else 0.0 for r in ref]
    for what, (k_max, k_rms), (y_max, y_rms), fl in zip(("param", "exp_avg", "exp_avg_sq"), _errors(kernel_state, ref), _errors(yard_state, ref), floor):
        y_max, y_rms = max(y_max, fl), max(y_rms, fl)
        r_max, r_rms = (k_max / y_max if y_max else float(k_max > 0)), (k_rms / y_rms if y_rms else float(k_rms > 0))
        print(f"[fit-kernels] {name} {what}: kernel max {k_max:.3e} rms {k_rms:.3e}; float32 torch max {y_max:.3e} rms {y_rms:.3e}; "
              f"ratios {r_max:.2f} {r_rms:.2f}")
        assert k_max <= factor * y_max and k_rms <= factor * y_rms, (name, what, k_max, y_max, k_rms, y_rms)
        worst = max(worst, r_max, r_rms)
    return worst


def _run_adam(name, n, steps, step0=0, p0=None, m0=None, v0=None, seed=0, t0=37):
    """``steps`` Adam steps after ``step0`` earlier ones on all paths from the same gradients: float64, float32 torch on the CPU,
    smil_adam_step, smil_adam_step_multi (one tensor) and smil_adam_step_dev with the device step count ahead by ``t0``."""
    eng = _engine()
    p_init, frozen, grads = _adam_problem(n, seed)
    p0 = p_init if p0 is None else p0
    m0 = torch.zeros(n) if m0 is None else m0
    v0 = torch.zeros(n) if v0 is None else v0
    yard = _Torch32(p0, LR, m0, v0, step0)
    host, multi, dev = ([_cu(p0).clone(), _cu(m0).clone(), _cu(v0).clone()] for _ in range(3))
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)

    def feed():
        for k, g in enumerate(grads(steps)):
            t = step0 + k + 1
            gd = _cu(g)
            yard.step(g)
            eng.adam_step(host[0], gd, host[1], host[2], LR, t, B1, B2, EPS)
            eng.adam_step_multi([(multi[0], gd, multi[1], multi[2], LR, t)], B1, B2, EPS)
            step_dev.fill_(t + t0)
            eng.adam_step_dev(dev[0], gd, dev[1], dev[2], LR, step_dev, t0, B1, B2, EPS)
            yield g

    ref = None
    for ref in fit_ref.adam_iter(p0, feed(), LR, B1, B2, EPS, m0, v0, step0):
        pass
    torch.cuda.synchronize()
    for a, b in zip(host, multi):
        assert torch.equal(a, b), f"{name}: adam_step_multi differs from adam_step"
    worst = max(_check_adam(f"{name} adam_step", host, yard.state(), ref), _check_adam(f"{name} adam_step_dev", dev, yard.state(), ref))
    if step0 == 0:
        for st in (host, dev):
            assert torch.equal(st[0].cpu()[frozen], p0[frozen]) and not st[1].cpu()[frozen].any() and not st[2].cpu()[frozen].any(), \
                f"{name}: an element without gradient moved"
    return worst


@pytest.mark.parametrize("steps", [1, 2, 10, 200])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 131073, 600001])
def test_adam(n, steps):
    _run_adam(f"adam[n={n}-steps={steps}]", n, steps)


def test_adam_continued_to_step_5000():
    """Steps 4801..5000 with the moments carried from a float64 run of the first 4800 (rounded to float32 once, for every path)."""
    n = 257
    p0, frozen, grads = _adam_problem(n, seed=11)
    for p, m, v in fit_ref.adam_iter(p0, grads(4800), LR, B1, B2, EPS):
        pass
    _run_adam("adam[continued 4801..5000]", n, 200, step0=4800, p0=p.float(), m0=m.float(), v0=v.float(), seed=12)


def test_adam_multi_many_tensors():
    """8 tensors of very different lengths (one of a single element), lr and step in ONE launch, and 9 through the wrapper's
    chunking: bit for bit what smil_adam_step gives tensor by tensor."""
    eng = _engine()
    lengths = [1, 37, 255, 256, 257, 1000, 131073, 600001, 5]
    for count in (8, 9):
        single, multi, meta = [], [], []
        for k, n in enumerate(lengths[:count]):
            p0, frozen, grads = _adam_problem(n, seed=20 + k)
            single.append([_cu(p0).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)])
            multi.append([_cu(p0).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)])
            meta.append((1e-3 * (k + 1), 1 + 3 * k, grads, p0, frozen))
        for it in range(3):
            items = []
            for s, m, (lr, step, grads, _, _) in zip(single, multi, meta):
                gd = _cu(next(grads(1)))
                eng.adam_step(s[0], gd, s[1], s[2], lr, step + it, B1, B2, EPS)
                items.append((m[0], gd, m[1], m[2], lr, step + it))
            eng.adam_step_multi(items, B1, B2, EPS)
        torch.cuda.synchronize()
        for k, (s, m, (_, _, _, p0, frozen)) in enumerate(zip(single, multi, meta)):
            for a, b in zip(s, m):
                assert torch.equal(a, b), f"tensor {k} of {count} (length {lengths[k]})"
            assert lengths[k] < 37 or not torch.equal(m[0].cpu(), p0)  # (a lone element may draw a gradient too small to move it)
            assert torch.equal(m[0].cpu()[frozen], p0[frozen]) and not m[1].cpu()[frozen].any() and not m[2].cpu()[frozen].any()


def test_adam_dev_step_offset_matches_host_step():
    """adam_step_dev with step_offset = t0 is adam_step at step = t - t0: both within the Adam bound of the same float64 run (checked
    in test_adam for t0 = 37), and here side by side for several offsets at the step where a wrong count matters most (t - t0 = 1)."""
    eng = _engine()
    n = 257
    p0, frozen, grads = _adam_problem(n, seed=30)
    g = next(grads(1))
    ref = fit_ref.adam(p0, [g], LR, B1, B2, EPS)[-1]
    yard = _Torch32(p0, LR)
    yard.step(g)
    for t0 in (0, 1, 199, 4999):
        st = [_cu(p0).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
        eng.adam_step_dev(st[0], _cu(g), st[1], st[2], LR, torch.tensor([t0 + 1], dtype=torch.int32, device=DEV), t0, B1, B2, EPS)
        torch.cuda.synchronize()
        _check_adam(f"adam_step_dev[t0={t0}]", st, yard.state(), ref)
