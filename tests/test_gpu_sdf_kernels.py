"""Kernel-level checks of the SDF-guided term against tests/sdf_ref.py: the K-nearest search exactly (ties included), the term and its
gradient, the edges of the z-score and the fixed-point scatter, and the vertex sampler.  No bound here comes from the kernels:
u = 2^-24 is float32's unit roundoff; 1e-5 (loss, gradient relative to the mesh's largest) is the bound of the chamfer tests."""
import functools
import os

import numpy as np
import pytest
import torch

import sdf_ref
from conftest import GOLDEN, MODEL_FILES
from mesh3d_ref import dyadic_clouds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
K_MAX = 64  # SMIL_KNN_MAX_K (asserted against the binding below)

SEARCH_SHAPES = [(1, 2, 2, 1), (1, 5, 50, 50), (1, 64, 51, 50), (2, 257, 255, 1), (2, 257, 256, 2), (3, 65, 257, 50),
                 (1, 300, 1030, K_MAX), (2, 1100, 4100, 50)]


def _report(what, **kw):
    print(f"[sdf] {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared clouds are read-only)


@functools.lru_cache(maxsize=None)
def _brute(N, P1, P2, K, swap=False):
    x, y = dyadic_clouds(N, P1, P2)
    out = sdf_ref.knn_brute(y, x, K) if swap else sdf_ref.knn_brute(x, y, K)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("N,P1,P2,K", SEARCH_SHAPES)
def test_search_is_exact_on_the_grid(N, P1, P2, K):
    from smilify_amd import _lib, engine

    assert _lib.KNN_MAX_K == K_MAX
    x, y = dyadic_clouds(N, P1, P2)
    both = K <= P1
    dx, ix, dy, iy, ins = engine.knn(_dev(x), _dev(y), K, both=both)
    tied = []
    for got_d, got_i, swap in ((dx, ix, False), (dy, iy, True)) if both else ((dx, ix, False),):
        rd, ri, nxt = _brute(N, P1, P2, K, swap)
        assert np.array_equal(got_i.cpu().numpy().astype(np.int64), ri)
        assert np.array_equal(got_d.double().cpu().numpy(), rd)  # (every distance on the grid is exact in float32)
        tied.append((nxt == rd[..., -1]).mean())
    _report(f"search {N, P1, P2, K}", share_kth_equals_next=float(np.mean(tied)), insertions_per_query=float(ins.item()) / (
        N * (P1 + (P2 if both else 0))))


@functools.lru_cache(maxsize=None)
def _scan_clouds():
    from smilify_amd import model_io

    def unit(v):
        v = np.asarray(v, np.float64)
        v = v - v.mean(0)
        return (v / np.abs(v).max()).astype(np.float32)

    a = unit(np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))["verts"])
    s = unit(model_io.load_model(MODEL_FILES["stick"]).v_template)
    assert len(a) >= 3000 and len(s) >= 3000
    pick = lambda v: v[np.linspace(0, len(v) - 1, 3000).astype(np.int64)][None]  # noqa: E731
    return pick(a), pick(s)


def test_search_off_the_grid():
    from smilify_amd import engine

    x, y = _scan_clouds()
    K = 50
    dx, ix, dy, iy, ins = engine.knn(_dev(x), _dev(y), K, both=True)
    for got_d, got_i, q, c in ((dx, ix, x, y), (dy, iy, y, x)):
        d, i = got_d.double().cpu().numpy()[0], got_i.cpu().numpy().astype(np.int64)[0]
        assert (np.diff(d, axis=1) >= 0).all()
        assert (np.sort(i, axis=1)[:, 1:] != np.sort(i, axis=1)[:, :-1]).all() and i.min() >= 0 and i.max() < c.shape[1]
        rd, _, _ = sdf_ref.knn_brute(q, c, K)
        assert np.abs(d - rd[0]).max() <= 1e-6
        at = ((q[0].astype(np.float64)[:, None, :] - c[0].astype(np.float64)[i]) ** 2).sum(-1)
        assert (np.abs(d - at) <= 4 * U * at).all()
    _report("scan search", insertions_per_query=float(ins.item()) / 6000)


def _grid_inputs(N, P1, P2, scale_bits):
    x, y = dyadic_clouds(N, P1, P2, seed=3)
    x, y = x.copy(), y.copy()
    if N > 1:
        x[1] *= 2.0 ** -scale_bits
        y[1] *= 2.0 ** -scale_bits
    rng = np.random.RandomState(11 + N)
    return x, y, rng.randn(N, P1).astype(np.float32), rng.randn(N, P2).astype(np.float32)


def _check_against_ref(x, y, xs, ys, K, psum, bsum, single, tag):
    from smilify_amd import engine

    loss, dx, dy, _, _ = engine.sdf_distance(_dev(x), _dev(y), _dev(xs), _dev(ys), K, single, psum, bsum)
    want, ix, iy = sdf_ref.sdf_term(x, y, xs, ys, K, psum, bsum, single)
    gx, gy = sdf_ref.sdf_grad_at(x, y, xs, ys, ix, iy, psum, bsum, single)
    got = float(loss.item())
    worst = 0.0
    for g, w in ((dx, gx), (dy, gy)):
        g = g.double().cpu().numpy()
        for n in range(x.shape[0]):
            top = np.abs(w[n]).max()
            err = np.abs(g[n] - w[n]).max()
            worst = max(worst, err / top if top > 0 else 0.0)
            assert err <= 1e-5 * top, (tag, n, err, top)
            assert (g[n][w[n] == 0] == 0).all(), (tag, n)
    _report(tag, loss_rel_err=abs(got - want) / abs(want), worst_grad_err_over_largest=worst)
    assert abs(got - want) <= 1e-5 * abs(want), (tag, got, want)


@pytest.mark.parametrize("N", [1, 3])
def test_term_on_the_grid(N):
    """Indices are exact on the grid, so loss and gradient compare with the float64 term directly."""
    x, y, xs, ys = _grid_inputs(N, 130, 257, 7)
    for psum in (False, True):
        for bsum in (False, True):
            for single in (False, True):
                _check_against_ref(x, y, xs, ys, 50, psum, bsum, single, f"grid N={N} psum={psum} bsum={bsum} single={single}")


def test_k1_is_the_chamfer_distance():
    from smilify_amd import engine, fit3d

    x, y, xs, ys = _grid_inputs(2, 257, 300, 0)
    for single in (False, True):
        loss, dx, dy, _, _ = engine.sdf_distance(_dev(x), _dev(y), _dev(xs), _dev(ys), 1, single, True, True)
        X, Y = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
        ch, _ = fit3d.chamfer_distance(X, Y, point_reduction="sum", batch_reduction="sum", single_directional=single)
        gx, gy = torch.autograd.grad(ch, (X, Y))
        assert torch.equal(loss.reshape(()), ch.detach())
        assert torch.equal(dx, gx) and torch.equal(dy, gy)


def test_constant_values():
    """A constant side has std 0, clamped: its z-scores are exactly 0.  With both sides constant every weight is 1/K and r_i is the
    mean of the K distances; with one side constant the other side's z-scores still weigh the neighbours."""
    from smilify_amd import engine

    x, y, xs, ys = _grid_inputs(2, 130, 257, 0)
    K = 8
    cx, cy = np.full_like(xs, 3.5), np.full_like(ys, -2.25)
    loss, _, _, tables, _ = engine.sdf_distance(_dev(x), _dev(y), _dev(cx), _dev(cy), K, False, True, True, want_tables=True)
    want = sum(float(t.double().mean(-1).sum()) for t in (tables[0], tables[2]))
    assert abs(float(loss.item()) - want) <= 1e-6 * want  # (exact sums on the grid, up to the float32 weights 1/K)
    dk, _, _ = sdf_ref.knn_brute(x, y, K)
    dk2, _, _ = sdf_ref.knn_brute(y, x, K)
    assert abs(float(loss.item()) - (dk.mean(-1).sum() + dk2.mean(-1).sum())) <= 1e-6 * want
    _check_against_ref(x, y, cx, ys, K, False, False, False, "constant x values")


def _random_inputs(k=0):
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 300, 3, generator=g) * 2 - 1) * 2.0 ** -k
    y = (torch.rand(2, 700, 3, generator=g) * 2 - 1) * 2.0 ** -k
    xs = 100 + 1e-2 * torch.randn(2, 300, generator=g)
    ys = 100 + 1e-2 * torch.randn(2, 700, generator=g)
    return x, y, xs, ys


def test_large_offset_values_against_float32_torch():
    """Values 100 + 1e-2 randn: the error against float64 at the kernel's indices beside that of float32 torch evaluating the same
    formula at the same indices, per mesh (the yardstick floored at half an ulp of the mesh's largest gradient)."""
    from smilify_amd import engine

    x, y, xs, ys = _random_inputs()
    _, dx, dy, tables, _ = engine.sdf_distance(x.to(DEV), y.to(DEV), xs.to(DEV), ys.to(DEV), 50, want_tables=True)
    ix, iy = tables[1].long().cpu(), tables[3].long().cpu()
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    want = torch.autograd.grad(sdf_ref.sdf_term_at(xr, yr, xs.double(), ys.double(), ix, iy), (xr, yr))
    x32, y32 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    yard = torch.autograd.grad(sdf_ref.sdf_term_at(x32, y32, xs, ys, ix, iy), (x32, y32))
    for got, w, f32 in zip((dx, dy), want, yard):
        for b in range(2):
            e_k = float((got[b].double().cpu() - w[b]).abs().max())
            e_y = max(float((f32[b].double() - w[b]).abs().max()), U * float(w[b].abs().max()))
            _report(f"offset 100, mesh {b}", kernel_err=e_k, float32_torch_err=e_y)
            assert e_k <= 4 * e_y, (b, e_k, e_y)


def test_power_of_two_scaling_is_exact():
    """The weights do not depend on the positions: clouds scaled by 2^-k give the loss times 2^-2k and the gradients times 2^-k, bit
    for bit (the fixed-point unit follows the data)."""
    from smilify_amd import engine

    base = None
    for k in (0, 10, 20):
        x, y, xs, ys = _random_inputs(k)
        xs, ys = xs - 100, ys - 100
        loss, dx, dy, tables, _ = engine.sdf_distance(x.to(DEV), y.to(DEV), xs.to(DEV), ys.to(DEV), 50, want_tables=True)
        if k == 0:
            base = (loss, dx, dy, tables)
            continue
        assert torch.equal(tables[1], base[3][1]) and torch.equal(tables[3], base[3][3])
        assert torch.equal(loss * 4.0 ** k, base[0]), (k, float(loss) * 4.0 ** k, float(base[0]))
        assert torch.equal(dx * 2.0 ** k, base[1]) and torch.equal(dy * 2.0 ** k, base[2]), k


def test_two_calls_give_the_same_bits():
    from smilify_amd import engine

    x, y, xs, ys = (t.to(DEV) for t in _random_inputs())
    a = engine.sdf_distance(x, y, xs, ys, 50)
    b = engine.sdf_distance(x, y, xs, ys, 50)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- vertex sampler ---------------------------------------------------------------------------------------------------------------
SAMPLER_V = (6, 3020)


def _sampler_inputs():
    g = torch.Generator().manual_seed(9)
    verts = torch.randn(sum(SAMPLER_V), 3, generator=g)
    vals = torch.randn(sum(SAMPLER_V), generator=g)
    off = torch.tensor([0, SAMPLER_V[0], sum(SAMPLER_V)], dtype=torch.int32)
    return verts, vals, off


@pytest.mark.parametrize("S", [255, 257])
def test_sampler_matches_the_restatement(S):
    from smilify_amd import engine

    verts, vals, off = _sampler_inputs()
    for seed in (0, 1, 1 << 32, (1 << 63) - 1):
        pts, val, idx = engine.sample_vertices(verts.to(DEV), vals.to(DEV), off.to(DEV), 2, S, seed)
        for n, V in enumerate(SAMPLER_V):
            want = sdf_ref.vertex_indices(n, S, seed, V)
            assert np.array_equal(idx[n].cpu().numpy().astype(np.int64), want), (seed, n)
            at = torch.from_numpy(want) + int(off[n])
            assert torch.equal(pts[n].cpu(), verts[at]) and torch.equal(val[n].cpu(), vals[at])


def test_sampler_gradient_sums_duplicates_deterministically():
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    verts, vals, off = _sampler_inputs()
    S = 257
    vl = [verts[:6].to(DEV).requires_grad_(True), verts[6:].to(DEV).requires_grad_(True)]
    meshes = Meshes(vl, [torch.zeros(1, 3, dtype=torch.int64, device=DEV)] * 2)
    probe = torch.randn(2, S, 3, generator=torch.Generator().manual_seed(2)) * torch.tensor([1.0, 2.0 ** -12]).view(2, 1, 1)
    grads = []
    for _ in range(2):
        pts, _, idx = fit3d.sample_vertices_with_index(meshes, [vals[:6], vals[6:]], S, seed=77)
        grads.append(torch.autograd.grad((pts * probe.to(DEV)).sum(), vl))
    for n in range(2):
        assert torch.equal(grads[0][n], grads[1][n])
        want, mag = np.zeros((SAMPLER_V[n], 3)), np.zeros((SAMPLER_V[n], 3))
        i = idx[n].cpu().numpy()
        np.add.at(want, i, probe[n].double().numpy())
        np.add.at(mag, i, probe[n].double().abs().numpy())
        assert (np.abs(grads[0][n].double().cpu().numpy() - want) <= 8 * U * mag).all()
    assert len(set(idx[0].tolist())) == 6  # (every vertex of the small mesh is drawn many times)


def test_sampler_gradient_scales_exactly_with_the_probe():
    """The fixed-point unit follows the mesh's largest |component|: a probe times 2^k gives the gradients times 2^k, bit for bit,
    and an all-zero probe (a recorded maximum of 0) exact zeros."""
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    verts, vals, off = _sampler_inputs()
    S = 257
    vl = [verts[:6].to(DEV).requires_grad_(True), verts[6:].to(DEV).requires_grad_(True)]
    meshes = Meshes(vl, [torch.zeros(1, 3, dtype=torch.int64, device=DEV)] * 2)
    probe = torch.randn(2, S, 3, generator=torch.Generator().manual_seed(2)) * torch.tensor([1.0, 2.0 ** -12]).view(2, 1, 1)

    def grads(p):
        pts, _, _ = fit3d.sample_vertices_with_index(meshes, [vals[:6], vals[6:]], S, seed=77)
        return torch.autograd.grad((pts * p.to(DEV)).sum(), vl)

    base = grads(probe)
    assert all(g.abs().sum() > 0 for g in base)
    for k in (-40, 0, 40):
        for g, b in zip(grads(probe * 2.0 ** k), base):
            assert torch.equal(g, b * 2.0 ** k), k
    for g in grads(torch.zeros_like(probe)):
        assert torch.equal(g, torch.zeros_like(g))
