"""The 3-D registration losses on the MI355X against the float64 oracle (tests/mesh3d_ref.py), and the fitter_3d drop-ins."""
import os

import numpy as np
import pytest
import torch

import mesh3d_ref as ref
from conftest import GOLDEN, MODEL_FILES, oracle_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _atta():
    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    v = torch.from_numpy(d["verts"]).double()
    v = v - v.mean(0)
    v = v / v.abs().max()
    return v.float(), torch.from_numpy(d["faces"].astype(np.int64))


def _posed(tables, B, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.from_numpy(tables.v_template)[None].repeat(B, 1, 1)
    return (v + 0.01 * torch.randn(v.shape, generator=g)).float()


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


# ---- regularisers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["stick", "mouse", "synthetic"])
@pytest.mark.parametrize("B", [1, 5])
def test_regularisers_against_oracle(tables, key, B):
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    t = tables(key)
    verts = _posed(t, B, seed=B)
    faces = torch.from_numpy(t.faces.astype(np.int64))
    m = Meshes(verts.to(DEV).requires_grad_(True), faces[None].repeat(B, 1, 1).to(DEV))
    lap_fn = ref.laplacian_loss_sparse
    for k, fn in enumerate((ref.edge_loss, ref.normal_loss, lap_fn)):
        v = m.verts_padded()
        out = fit3d.mesh_regularisers(m, k == 0, k == 1, k == 2)
        (g,) = torch.autograd.grad(out[k], v)
        rl, rg = ref.with_grad(fn, verts, t.faces)
        assert _rel(float(out[k]), rl) <= 1e-5, (key, k, float(out[k]), rl)
        err = (g.double().cpu() - rg).abs().max() / rg.abs().max()
        assert err <= 1e-5, (key, k, float(err))
    # the three drop-ins are the same numbers
    for fn, k in ((fit3d.mesh_edge_loss, 0), (fit3d.mesh_normal_consistency, 1), (fit3d.mesh_laplacian_smoothing, 2)):
        assert float(fn(m)) == float(fit3d.mesh_regularisers(m)[k])


# ---- chamfer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["stick", "mouse"])
@pytest.mark.parametrize("B", [1, 7])
def test_chamfer_against_oracle(tables, key, B):
    from smilify_amd import engine

    t = tables(key)
    g = torch.Generator().manual_seed(11 + B)
    y = _posed(t, B, seed=3)
    lo, hi = y.amin((0, 1)), y.amax((0, 1))
    x = (lo + (hi - lo) * torch.rand(B, 3000, 3, generator=g)).float()
    loss, ix, iy, dx, dy = engine.chamfer(x.to(DEV), y.to(DEV))
    x64, y64 = x.double(), y.double()
    rloss, rix, riy = ref.chamfer(x64, y64)
    assert _rel(float(loss), float(rloss)) <= 1e-5
    # every argmin's distance within 1e-6 relative of the float64 minimum
    ix, iy = ix.long().cpu(), iy.long().cpu()
    dgx = ((x64 - torch.gather(y64, 1, ix[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    dmx = ((x64 - torch.gather(y64, 1, rix[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    assert ((dgx - dmx) <= 1e-6 * dmx + 1e-12).all()
    dgy = ((y64 - torch.gather(x64, 1, iy[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    dmy = ((y64 - torch.gather(x64, 1, riy[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    assert ((dgy - dmy) <= 1e-6 * dmy + 1e-12).all()
    # gradients: the float64 gradient at the GPU's indices
    xr, yr = x64.clone().requires_grad_(True), y64.clone().requires_grad_(True)
    gx, gy = torch.autograd.grad(ref.chamfer_at(xr, yr, ix, iy), (xr, yr))
    for got, want in ((dx, gx), (dy, gy)):
        err = (got.double().cpu() - want).abs().max() / want.abs().max()
        assert err <= 1e-5, float(err)


def test_chamfer_reductions_and_drop_in(tables):
    from smilify_amd import fit3d

    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 500, 3, generator=g)
    y = torch.randn(3, 700, 3, generator=g)
    for sd in (False, True):
        for pr in ("mean", "sum"):
            for br in ("mean", "sum"):
                xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
                loss, none = fit3d.chamfer_distance(xg, yg, point_reduction=pr, batch_reduction=br, single_directional=sd)
                assert none is None and loss.dim() == 0
                rl = ref.chamfer(x.double(), y.double(), sd, pr == "sum", br == "sum")[0]
                assert _rel(float(loss), float(rl)) <= 1e-5, (sd, pr, br)
                gx, gy = torch.autograd.grad(3.0 * loss, (xg, yg))
                xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
                rl2 = ref.chamfer_at(xr, yr, *ref.chamfer(xr.detach(), yr.detach())[1:], single_directional=sd, point_sum=pr == "sum",
                                     batch_sum=br == "sum")
                wx, wy = torch.autograd.grad(3.0 * rl2, (xr, yr))
                assert (gx.double().cpu() - wx).abs().max() <= 1e-5 * wx.abs().max(), (sd, pr, br)
                assert (gy.double().cpu() - wy).abs().max() <= 1e-5 * wy.abs().max(), (sd, pr, br)  # (single_directional: y gets x's argmins)


# ---- sampling -----------------------------------------------------------------------------------------------------------------
def test_sampling_area_frequencies_and_containment():
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    # two triangles, area 0.5 : 1.5
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [2, 3, 0]])
    f = torch.tensor([[0, 1, 2], [3, 4, 5]])
    m = Meshes([v.to(DEV)], [f.to(DEV)])
    S = 1 << 20
    pts, face = fit3d.sample_points_with_faces(m, S, seed=1234)
    face = face.cpu().long()[0]
    n1 = int((face == 1).sum())
    p = 0.75
    assert abs(n1 - p * S) <= 5 * np.sqrt(S * p * (1 - p)), n1
    # every sample inside its triangle: barycentric coordinates >= 0 (to rounding)
    P = pts[0].cpu().double()
    tri = v.double()[f[face]]  # (S,3,3)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    v0, v1, v2 = b - a, c - a, P - a
    d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
    d20, d21 = (v2 * v0).sum(1), (v2 * v1).sum(1)
    den = d00 * d11 - d01 * d01
    bv = (d11 * d20 - d01 * d21) / den
    bw = (d00 * d21 - d01 * d20) / den
    assert (bv >= -1e-6).all() and (bw >= -1e-6).all() and (bv + bw <= 1 + 1e-6).all()
    assert (P[:, 2] == 0).all()


def test_sampling_mean_matches_area_centroid_and_seeds():
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    v, f = _atta()
    m = Meshes([v.to(DEV)], [f.to(DEV)])
    pts = fit3d.sample_points_with_faces(m, 1 << 20, seed=7)[0][0].cpu().double()
    vv = v.double()
    tri = vv[f]
    area = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)
    centroid = (area[:, None] * tri.mean(1)).sum(0) / area.sum()
    # spread of one sample about the centroid bounds the error of the mean
    sd = ((pts - centroid) ** 2).sum(1).mean().sqrt()
    assert (pts.mean(0) - centroid).norm() <= 5 * sd / np.sqrt(pts.shape[0]), (pts.mean(0), centroid)
    a1 = fit3d.sample_points_with_faces(m, 3000, seed=99)[0]
    a2 = fit3d.sample_points_with_faces(m, 3000, seed=99)[0]
    a3 = fit3d.sample_points_with_faces(m, 3000, seed=100)[0]
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)
    torch.manual_seed(3)
    b1 = fit3d.sample_points_from_meshes(m, 3000)
    torch.manual_seed(3)
    b2 = fit3d.sample_points_from_meshes(m, 3000)
    assert torch.equal(b1, b2)
    with pytest.raises(NotImplementedError):
        fit3d.sample_points_from_meshes(Meshes([v.to(DEV).requires_grad_(True)], [f.to(DEV)]), 10)


def test_heterogeneous_target_batch(tables):
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    v, f = _atta()
    st = tables("stick")
    v2 = torch.from_numpy(st.v_template)
    f2 = torch.from_numpy(st.faces.astype(np.int64))
    m = Meshes([v.to(DEV), v2.to(DEV)], [f.to(DEV), f2.to(DEV)])
    pts, face = fit3d.sample_points_with_faces(m, 4000, seed=5)
    face = face.cpu().long()
    assert face[0].max() < f.shape[0] and face[1].max() < f2.shape[0] and face.min() >= 0
    # each mesh's points lie in its own faces' planes: distance to the chosen face's plane ~ 0
    for k, (vv, ff) in enumerate(((v, f), (v2, f2))):
        tri = vv.double()[ff[face[k]]]
        n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        n = n / n.norm(dim=1, keepdim=True).clamp(min=1e-30)
        dist = ((pts[k].cpu().double() - tri[:, 0]) * n).sum(1).abs()
        assert float(dist.max()) < 1e-5 * float(vv.abs().max()), k


def test_losses_are_bit_reproducible(tables):
    from smilify_amd import engine
    from smilify_amd.mesh3d import Meshes

    t = tables("mouse")
    y = _posed(t, 7, seed=1).to(DEV)
    x = (torch.rand(7, 3000, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)
    r1 = engine.chamfer(x, y)
    r2 = engine.chamfer(x, y)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    m = Meshes(y, torch.from_numpy(t.faces.astype(np.int64))[None].repeat(7, 1, 1).to(DEV))
    topo = m.topology().device(DEV)
    o1 = engine.mesh_regularisers(topo, y, 7)
    o2 = engine.mesh_regularisers(topo, y, 7)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)


# ---- Stage / SMAL3DFitter -------------------------------------------------------------------------------------------------------
def _fitter(B, key="stick"):
    from smilify_amd import fit3d

    return fit3d.SMAL3DFitter(batch_size=B, device=DEV, model_path=MODEL_FILES[key])


def test_stage_step_gradients_against_oracle(tables):
    from oracle import lbs_ref
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    B = 2
    t = tables("stick")
    model = _fitter(B)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():  # a non-trivial point to differentiate at
        for name in ("betas", "log_beta_scales", "betas_trans", "global_rot", "trans", "joint_rot", "deform_verts"):
            p = getattr(model, name)
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    v, f = _atta()
    targets = Meshes([v.to(DEV)] * B, [f.to(DEV)] * B)
    stage = fit3d.Stage(1, "all", model, targets, lr=0.0, loss_weights=dict(w_edge=1.0, w_normal=0.01, w_laplacian=0.1))
    stage.optimizer.zero_grad()
    stage.step(0)
    got = {n: getattr(model, n).grad.detach().double().cpu() for n in fit3d.SMALParamGroup.param_map["all"]}
    # oracle: float64 LBS + the float64 losses on the step's own samples
    om = {k: (v_.double() if torch.is_tensor(v_) and v_.is_floating_point() else v_) for k, v_ in oracle_model(t).items()}
    params = {n: getattr(model, n).detach().double().cpu().clone().requires_grad_(True) for n in got}
    theta = torch.cat([params["global_rot"][:, None], params["joint_rot"]], 1)
    out = lbs_ref.smal_forward(om, params["betas"], theta, trans=params["trans"], betas_logscale=params["log_beta_scales"],
                               betas_trans=params["betas_trans"], allow_limb_scaling=model.smal_model.config.ALLOW_LIMB_SCALING)
    verts = out["verts"] + params["deform_verts"]
    tgt = stage.last_target_samples.double().cpu()
    _, ix, iy = ref.chamfer(tgt, verts.detach())
    loss = (ref.chamfer_at(tgt, verts, ix, iy) + ref.edge_loss(verts, t.faces) + 0.01 * ref.normal_loss(verts, t.faces)
            + 0.1 * ref.laplacian_loss_sparse(verts, t.faces))
    want = dict(zip(got, torch.autograd.grad(loss, [params[n] for n in got])))
    for n in got:
        a, b = got[n].reshape(-1), want[n].reshape(-1)
        rel = float((a - b).norm() / b.norm())
        cos = float((a @ b) / (a.norm() * b.norm()))
        assert rel <= 1e-4 and cos >= 0.99999, (n, rel, cos)


def test_registration_recovers_rigid_offset():
    """An init stage (global_rot, trans) moves the STICK model onto a copy of itself shifted by a known offset.  The bound: a float64
    CPU run of the same stage (same offset, lr, iterations, torch.multinomial / torch.rand samples, seed 0) ends at
    |trans - offset| = 3.3e-4 of |offset| = 6.2e-2; the HIP run draws other samples, so it is allowed 10x that."""
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    torch.manual_seed(0)
    model = _fitter(1)
    offset = torch.tensor([0.05, -0.03, 0.02], device=DEV)
    with torch.no_grad():
        tv = model() + offset
    target = Meshes([tv[0]], [model.faces[0]])
    stage = fit3d.Stage(150, "init", model, target, lr=0.005)
    stage.run()
    err = float((model.trans.detach()[0] - offset).norm())
    assert err <= REG_BOUND, err
    ch = stage.loss_components_to_plot["chamfer"]
    assert float(ch[-1]) < 0.2 * float(ch[0]), (float(ch[0]), float(ch[-1]))


REG_BOUND = 3.3e-3


def test_drop_in_contract(tmp_path):
    from smilify_amd import fit3d

    assert fit3d.SMALParamGroup.param_map["init"] == ["global_rot", "trans"]
    assert fit3d.SMALParamGroup.param_map["deform"] == ["deform_verts"]
    v, f = _atta()
    d = tmp_path / "meshes"
    d.mkdir()
    for k, s in enumerate((1.0, 1.3)):
        with open(d / f"m{k}.obj", "w") as fh:
            for p in (v * s).tolist():
                fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
            for q in (f + 1).tolist():
                fh.write(f"f {q[0]} {q[1]} {q[2]}\n")
    out = tmp_path / "res"
    args = fit3d.build_parser().parse_args(["--model", MODEL_FILES["stick"], "--mesh_dir", str(d), "--nits", "3", "--results_dir", str(out),
                                            "--scheme", "init", "--batch_size", "1"])
    assert fit3d.main(args) == ["stage"]
    r = np.load(out / "stage.npz")
    assert set(r.files) == {"global_rot", "joint_rot", "betas", "log_beta_scales", "trans", "deform_verts", "betas_trans", "verts", "faces",
                            "labels"}
    assert r["trans"].shape == (2, 3) and r["verts"].shape[0] == 2 and list(r["labels"]) == ["m0.obj", "m1.obj"]
    assert not os.path.exists(out / "stage_batch_0.npz")
