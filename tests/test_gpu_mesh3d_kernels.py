"""The kernels of ``smilify_amd/csrc/mesh3d.hip`` against exact and float64 references (``tests/mesh3d_ref.py``) at the sizes and
edges where they can go wrong: the sampler against a step-by-step restatement, the chamfer search and gradients on a dyadic grid
where float32 is exact, off the grid with a per-mesh yardstick, and the regularisers on hand meshes.

Bounds (none is taken from the kernels; u = 2^-24):

* sampler: the face index equals the restatement's for every sample (integer and float64 arithmetic on identical inputs); every
  point within ``8 u max|coordinate of its face|`` of the point the restated float32 weights give in float64 (one rounding in
  sqrtf, one per weight, three in the sum, contracted or not);
* chamfer on the dyadic grid (multiples of 1/8 in [-1, 1]^3): indices equal numpy's first-occurrence argmin of the float64 rows
  for every query; the sum / sum loss equals the float64 value exactly (every minimum is a multiple of 1/64 and the sums stay below
  2^24 / 64), the other reductions within ``8 u`` relative (two roundings in the weight, one in the product, a few in the sum);
  every gradient element within ``8 u (|owned part| + |scattered part|)`` (at most five roundings; the fixed-point sums are exact
  on this grid), which is exactly 0 where both parts are 0;
* chamfer off the grid: every argmin's distance within 1e-6 of the float64 minimum, gradients within 1e-5 of each MESH's own largest
  gradient; and the gradient's error against float64 at most 4 x that of float32 torch evaluating ``ref.chamfer_at`` at the same
  indices (floored at half an ulp of the mesh's largest gradient), with the clouds scaled by 2^-k.  Scaling by a power of two
  changes no rounding anywhere (below the overflow and above the underflow of float32), so the scaled gradients must be the
  unscaled ones times 2^-k bit for bit;
* regularisers: losses within 1e-5 relative (plus 1e-13, the float64 reference's own rounding on O(1) terms, which decides only
  where the exact value is 0), gradients within 1e-5 of each mesh's own largest gradient, exactly 0 where that is 0.

Measured on an MI355X (``pytest -s`` prints every figure; the table is in DESIGN.md section 4.4): sampler points reach 0.25 of their
bound, dyadic gradients 0.21 of theirs; the chamfer gradient's error is 1.94 x float32 torch's on the worst mesh at every scale from
2^0 to 2^-50, with identical bits; the regularisers' per-mesh gradient errors stay below 5.5e-7.  With the fixed 2^-32 unit that
``k_chamfer_owned`` used before, the scale sweep fails at 2^-10 (smallest mesh: 4.9e-13 against a yardstick of 3.8e-14, 12.8 x).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mesh3d_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _report(name, **figures):
    print(f"[mesh3d-kernels] {name}: " + "  ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


# ---- sampler ------------------------------------------------------------------------------------------------------------------
TWO_TRI = (torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [2, 3, 0]]), torch.tensor([[0, 1, 2], [3, 4, 5]]))
SEEDS = (0, 1, 1 << 32, (1 << 63) - 1, 0x1234ABCD9E3779B9)


@functools.lru_cache(maxsize=None)
def _atta():
    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    v = torch.from_numpy(d["verts"]).double()
    v = v - v.mean(0)
    v = v / v.abs().max()
    return v.float(), torch.from_numpy(d["faces"].astype(np.int64))


def _meshes(*vf):
    from smilify_amd.mesh3d import Meshes

    return Meshes([v.to(DEV) for v, _ in vf], [f.to(DEV) for _, f in vf])


def _check_sampler(m, S, seed, name):
    """Every sample of ``m`` against the restatement on the same tables: faces exactly, points within the derived bound."""
    from smilify_amd import fit3d

    pts, face = fit3d.sample_points_with_faces(m, S, seed=seed)
    faces, off, cum = (t.cpu().numpy() for t in m.sampling_tables())
    rp, rf, fmax = ref.sample_points(m.verts_packed().detach().float().cpu().numpy(), faces, off, cum, S, seed)
    face, pts = face.cpu().numpy().astype(np.int64), pts.cpu().double().numpy()
    assert face.shape == rf.shape and pts.shape == rp.shape
    assert np.array_equal(face, rf), (name, seed, int((face != rf).sum()))
    err, bound = np.abs(pts - rp).max(-1), 8 * U * fmax
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    _report(f"sampler {name} S={S} seed={seed:#x}", point_error_over_bound=worst)
    assert (err <= bound).all(), (name, seed, worst)
    return pts, face


@pytest.mark.parametrize("S", [1, 255, 256, 257, 1000])
def test_sampler_equals_restatement(S):
    m = _meshes(TWO_TRI)
    seen = []
    for seed in SEEDS:
        pts, _ = _check_sampler(m, S, seed, "two_triangles")
        assert not any(np.array_equal(pts, p) for p in seen), seed  # (0 and 2^32 differ only in the high word)
        seen.append(pts)


def test_sampler_high_seed_word_and_mesh_index_enter_the_stream():
    m = _meshes(TWO_TRI, TWO_TRI)  # identical geometry twice
    a, _ = _check_sampler(m, 257, 5, "twins")
    b, _ = _check_sampler(m, 257, 5 + (7 << 32), "twins")
    assert not np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(b[0], b[1])


def test_sampler_never_chooses_zero_area_faces():
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [0.25, 2, 1]])
    # repeated indices: the area is exactly 0 in float64.  Zero-area faces first, in the middle (two in a row) and last
    f = torch.tensor([[0, 0, 1], [0, 1, 2], [2, 2, 2], [3, 1, 3], [1, 3, 2], [2, 3, 4], [3, 4, 3]])
    dead = [0, 2, 3, 6]
    m = _meshes((v, f))
    cum = m.sampling_tables()[2].cpu().numpy()
    assert cum[0] == 0 and cum[1] == cum[2] == cum[3] and cum[5] == cum[6] == 1.0
    for seed in SEEDS:
        _, face = _check_sampler(m, 1000, seed, "zero_area")
        assert not np.isin(face, dead).any()
        assert set(np.unique(face).tolist()) == {1, 4, 5}


def test_sampler_face_search_is_strict_at_a_table_entry():
    """Hand-built tables whose entries ARE the face uniforms of some samples: such a sample takes the first face whose cumulative
    area exceeds its uniform, that is the next one."""
    from smilify_amd import engine

    S, seed = 300, 0xC0FFEE1234567
    uf, _, _ = ref.sample_draws(0, S, seed)
    picked = np.sort(uf[[3, 64, 65, 255, 256, 299]])
    assert len(np.unique(picked)) == 6 and picked[-1] < 1.0
    cum = np.concatenate([picked, [1.0]])
    F = len(cum)
    verts = torch.tensor([[0.0, 0, 0]] + [[np.cos(k), np.sin(k), 0.125 * k] for k in range(F + 1)], dtype=torch.float32)
    faces = torch.tensor([[0, k + 1, k + 2] for k in range(F)], dtype=torch.int32)
    off = torch.tensor([0, F], dtype=torch.int32)
    pts, face = engine.sample_points(verts.to(DEV), faces.to(DEV), off.to(DEV), torch.from_numpy(cum).to(DEV), 1, S, seed, want_faces=True)
    rp, rf, fmax = ref.sample_points(verts.numpy(), faces.numpy(), off.numpy(), cum, S, seed)
    face = face.cpu().numpy().astype(np.int64)
    assert np.array_equal(face, rf)
    for k, value in enumerate(picked):
        s = int(np.nonzero(uf == value)[0][0])
        assert face[0, s] == k + 1, (k, s)
    assert (np.abs(pts.cpu().double().numpy() - rp).max(-1) <= 8 * U * fmax).all()


def test_sampler_heterogeneous_batch(tables):
    st = tables("stick")
    stick = (torch.from_numpy(st.v_template), torch.from_numpy(st.faces.astype(np.int64)))
    m = _meshes(TWO_TRI, _atta(), stick)
    for seed in (3, SEEDS[-1]):
        _, face = _check_sampler(m, 257, seed, "two_triangles+atta+stick")
        assert face[0].max() < 2 and face[1].max() < _atta()[1].shape[0] and face[2].max() < stick[1].shape[0]


def test_sampler_meshes_without_faces_or_area():
    from smilify_amd import fit3d

    v3 = torch.tensor([[1.0, 2, 3], [4, 5, 6], [7, 8, 10]])
    no_faces = (v3, torch.zeros(0, 3, dtype=torch.int64))
    no_area = (v3, torch.tensor([[0, 0, 1], [2, 2, 2]]))
    m = _meshes(no_faces, no_area, TWO_TRI)
    pts, face = _check_sampler(m, 257, 11, "empty+flat+two_triangles")
    assert (pts[:2] == 0).all() and (face[:2] == -1).all() and (face[2] >= 0).all()
    # the poisoned outputs of a second call are overwritten too (zeros are written, not left)
    p2, f2 = fit3d.sample_points_with_faces(m, 257, seed=11)
    assert torch.equal(p2.cpu().double(), torch.from_numpy(pts)) and (f2[:2] == -1).all()


# ---- chamfer on the dyadic grid -------------------------------------------------------------------------------------------------
REDUCTIONS = [(False, False), (False, True), (True, False), (True, True)]  # (point_sum, batch_sum)
DYADIC_CASES = ref.DYADIC_SHAPES + [(3, 5, 2500, True, 1), (2, 257, 1023, True, 1), (3, 2048, 2100, True, 2)]


def _case_id(c):
    return f"N{c[0]}-P{c[1]}x{c[2]}-{'single' if c[3] else 'both'}-splits{c[4]}"


def _chamfer(x, y, **kw):
    from smilify_amd import engine

    return engine.chamfer(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(y)).to(DEV), **kw)


def _check_grid_gradients(x, y, ix, iy, dx, dy, sd, ps, bs, what):
    parts = ref.chamfer_grad_parts(x, y, ix, iy, sd, ps, bs)
    worst = 0.0
    for got, own, sc in ((dx, parts[0], parts[1]), (dy, parts[2], parts[3])):
        got = got.cpu().double().numpy()
        err, bound = np.abs(got - (own + sc)), 8 * U * (np.abs(own) + np.abs(sc))
        assert (got[bound == 0] == 0).all(), what
        assert (err <= bound).all(), (what, float((err / np.where(bound > 0, bound, 1)).max()))
        worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    return worst


@pytest.mark.parametrize("case", DYADIC_CASES, ids=_case_id)
def test_chamfer_on_dyadic_grid(case):
    N, P1, P2, sd, splits = case
    assert ref.chamfer_splits(N, P1, P2, sd) == splits
    x, y = ref.dyadic_clouds(N, P1, P2)
    r = ref.dyadic_reference(N, P1, P2)
    if min(P1, P2) >= ref.TIE_QUOTA_MIN_P:
        assert ref.tie_fraction(r, sd) >= 0.10
    assert (r["dx"].sum() + r["dy"].sum()) * 64 < 2 ** 24  # every float32 sum of these multiples of 1/64 is exact
    worst = 0.0
    for ps, bs in REDUCTIONS:
        loss, ix, iy, dx, dy = _chamfer(x, y, single_directional=sd, point_sum=ps, batch_sum=bs)
        ix = ix.cpu().numpy().astype(np.int64)
        assert np.array_equal(ix, r["ix"]), (ps, bs, int((ix != r["ix"]).sum()))
        if sd:
            assert iy is None
            iy = r["iy"]  # (unused by the single-directional reference)
        else:
            iy = iy.cpu().numpy().astype(np.int64)
            assert np.array_equal(iy, r["iy"]), (ps, bs, int((iy != r["iy"]).sum()))
        want = ref.chamfer_loss_from(r["dx"], r["dy"], sd, ps, bs)
        if ps and bs:
            assert float(loss) == want, (float(loss), want)  # which pins every key's distance: all sums are exact
        else:
            assert abs(float(loss) - want) <= 8 * U * want, (ps, bs, float(loss), want)
        worst = max(worst, _check_grid_gradients(x, y, ix, iy, dx, dy, sd, ps, bs, (ps, bs)))
        # without gradients: no gradient outputs, and nothing else changes
        l2, ix2, iy2, dx2, dy2 = _chamfer(x, y, single_directional=sd, point_sum=ps, batch_sum=bs, want_grad=False)
        assert dx2 is None and dy2 is None and torch.equal(l2, loss) and np.array_equal(ix2.cpu().numpy(), ix)
        assert (iy2 is None) if sd else np.array_equal(iy2.cpu().numpy(), iy)
    _report(f"dyadic {_case_id(case)}", gradient_error_over_bound=worst, tied=float(ref.tie_fraction(r, sd)))


@pytest.mark.parametrize("sd", [False, True], ids=["both", "single"])
def test_chamfer_duplicate_across_split_boundary(sd):
    """The same coordinates at candidate index chunk - 1 and chunk (the last of one split, the first of the next): the merge of the
    splits must give the smaller index, as one sequential scan with < does."""
    N, P = 1, 4100
    splits = ref.chamfer_splits(N, P, P, sd)
    chunk = ref.chamfer_chunk(P, splits)
    assert (splits, chunk) == (4, 1280)
    x, y = (a.copy() for a in ref.dyadic_clouds(N, P, P, seed=1))
    marks = [(2.0, 2.0, 2.0), (-2.0, 2.0, 2.0), (2.0, -2.0, 2.0)]  # outside the grid: nothing else is as near
    for k, mark in enumerate(marks):
        b = (k + 1) * chunk
        y[0, b - 1] = y[0, b] = mark  # candidates of direction 0
        x[0, 7 + k] = mark            # their query
        if not sd:
            mark_x = tuple(-c for c in mark)
            x[0, b - 1] = x[0, b] = mark_x  # candidates of direction 1
            y[0, 11 + k] = mark_x
    r = ref.chamfer_brute(x, y)
    loss, ix, iy, _, _ = _chamfer(x, y, single_directional=sd, point_sum=True, batch_sum=True)
    ix = ix.cpu().numpy().astype(np.int64)
    for k in range(3):
        assert r["ix"][0, 7 + k] == (k + 1) * chunk - 1 and r["nx"][0, 7 + k] == 2
        assert ix[0, 7 + k] == (k + 1) * chunk - 1, (k, ix[0, 7 + k])
    assert np.array_equal(ix, r["ix"])
    if not sd:
        iy = iy.cpu().numpy().astype(np.int64)
        for k in range(3):
            assert iy[0, 11 + k] == (k + 1) * chunk - 1, (k, iy[0, 11 + k])
        assert np.array_equal(iy, r["iy"])
    assert float(loss) == ref.chamfer_loss_from(r["dx"], r["dy"], sd, True, True)


def test_chamfer_call_order_leaves_no_trace():
    """A call without gradients, one with gradients at another shape (free to reuse the first one's memory), the first again."""
    xa, ya = ref.dyadic_clouds(1, 4100, 4100)
    xb, yb = ref.dyadic_clouds(3, 2048, 2100)
    first = _chamfer(xa, ya, want_grad=False)
    first = [None if t is None else t.clone() for t in first]
    mid = _chamfer(xb, yb, want_grad=True)
    assert mid[3] is not None
    del mid
    third = _chamfer(xa, ya, want_grad=False)
    for a, b in zip(first, third):
        assert (a is None and b is None) or torch.equal(a, b)
    with_grad = _chamfer(xa, ya, want_grad=True)
    for a, b in zip(first[:3], with_grad[:3]):
        assert torch.equal(a, b)


# ---- chamfer off the grid -------------------------------------------------------------------------------------------------------
def _random_clouds(k=0, N=3, P1=500, P2=700):
    """float32 clouds with mesh b scaled by 2^-b (so that no mesh hides behind a larger one), all scaled by 2^-k (exactly)."""
    g = torch.Generator().manual_seed(17)
    x, y = torch.randn(N, P1, 3, generator=g), torch.randn(N, P2, 3, generator=g)
    s = (2.0 ** -torch.arange(N, dtype=torch.float32))[:, None, None] * 2.0 ** -k
    return (x * s).contiguous(), (y * s).contiguous()


def _gather_dist(q, c, idx):
    return ((q - torch.gather(c, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)


@pytest.mark.parametrize("sd", [False, True], ids=["both", "single"])
@pytest.mark.parametrize("ps,bs", REDUCTIONS)
def test_chamfer_off_grid_per_mesh(sd, ps, bs):
    from smilify_amd import engine

    x, y = _random_clouds()
    loss, ix, iy, dx, dy = engine.chamfer(x.to(DEV), y.to(DEV), single_directional=sd, point_sum=ps, batch_sum=bs)
    x64, y64 = x.double(), y.double()
    rloss, rix, riy = ref.chamfer(x64, y64, sd, ps, bs)
    assert abs(float(loss) - float(rloss)) <= 1e-5 * float(rloss)
    ix = ix.long().cpu()
    got, best = _gather_dist(x64, y64, ix), _gather_dist(x64, y64, rix)
    assert ((got - best) <= 1e-6 * best + 1e-12).all()
    if sd:
        iy = riy
    else:
        iy = iy.long().cpu()
        got, best = _gather_dist(y64, x64, iy), _gather_dist(y64, x64, riy)
        assert ((got - best) <= 1e-6 * best + 1e-12).all()
    xr, yr = x64.clone().requires_grad_(True), y64.clone().requires_grad_(True)
    gx, gy = torch.autograd.grad(ref.chamfer_at(xr, yr, ix, iy, sd, ps, bs), (xr, yr))
    for name, got, want in (("d_x", dx, gx), ("d_y", dy, gy)):
        for b in range(x.shape[0]):
            err = float((got[b].double().cpu() - want[b]).abs().max() / want[b].abs().max())
            assert err <= 1e-5, (name, b, err)


SCALE_ASSERTED = (0, 10, 20)
SCALE_MEASURED = (0, 10, 20, 30, 40, 50)


def test_chamfer_gradient_scale_sweep():
    """How far down in scale the scattered (fixed-point) side of the gradient holds: the error against float64 beside that of
    float32 torch on the same inputs at the same indices, per mesh; asserted within 4 x at 2^0, 2^-10 and 2^-20, measured further.
    Power-of-two scaling changes no rounding, so the gradients at 2^-k are those at 2^0 times 2^-k bit for bit."""
    from smilify_amd import engine

    base = None
    for k in SCALE_MEASURED:
        x, y = _random_clouds(k)
        _, ix, iy, dx, dy = engine.chamfer(x.to(DEV), y.to(DEV))
        ix, iy = ix.long().cpu(), iy.long().cpu()
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        want = torch.autograd.grad(ref.chamfer_at(xr, yr, ix, iy), (xr, yr))
        x32, y32 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        yard = torch.autograd.grad(ref.chamfer_at(x32, y32, ix, iy), (x32, y32))
        worst = 0.0
        for got, w, f32 in zip((dx, dy), want, yard):
            for b in range(x.shape[0]):
                e_k = float((got[b].double().cpu() - w[b]).abs().max())
                e_y = max(float((f32[b].double() - w[b]).abs().max()), U * float(w[b].abs().max()))
                worst = max(worst, e_k / e_y)
                if k in SCALE_ASSERTED:
                    assert e_k <= 4 * e_y, (k, b, e_k, e_y)
        rel = [float((got.double().cpu() - w).abs().max() / w.abs().max()) for got, w in zip((dx, dy), want)]
        rel32 = [float((f.double() - w).abs().max() / w.abs().max()) for f, w in zip(yard, want)]
        _report(f"scale sweep 2^-{k}", kernel_rel_err=max(rel), float32_torch_rel_err=max(rel32), worst_ratio_per_mesh=worst)
        if k == 0:
            base = (ix, iy, dx.cpu(), dy.cpu())
        elif k in SCALE_ASSERTED:
            assert torch.equal(ix, base[0]) and torch.equal(iy, base[1])
            assert torch.equal(dx.cpu() * 2.0 ** k, base[2]) and torch.equal(dy.cpu() * 2.0 ** k, base[3]), k


# ---- regularisers ---------------------------------------------------------------------------------------------------------------
REG_FNS = (ref.edge_loss, ref.normal_loss, ref.laplacian_loss_sparse)
MESHES = ref.hand_meshes()


def _topology(faces, V):
    from smilify_amd.mesh3d import Topology

    return Topology(faces, V).device(DEV)


def _batch(verts, scales):
    """(B,V,3) float32: mesh b is ``verts`` times scales[b] (powers of two: exact)."""
    return torch.from_numpy(verts)[None] * torch.tensor(scales, dtype=torch.float32)[:, None, None]


def _poisoned_call(topo, verts, terms):
    """engine.mesh_regularisers after blocks of the workspace's size were filled with NaN bit patterns and freed, so that what the
    call is given holds no earlier call's partial sums."""
    from smilify_amd import _lib, engine

    n = int(_lib.load().smil_mesh_reg_workspace_bytes(ctypes.byref(topo.struct), int(verts.shape[0])))
    junk = [torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(3)]
    del junk
    return engine.mesh_regularisers(topo, verts, terms)


def _check_reg_against_reference(name, verts_b, faces, out, grads, terms=7):
    """out3 and the per-mesh gradients of the terms in ``terms`` against float64 autograd on the same float32 inputs."""
    worst = 0.0
    for k, fn in enumerate(REG_FNS):
        if not terms & (1 << k):
            continue
        rl, rg = ref.with_grad(fn, verts_b, faces)
        assert abs(float(out[k]) - rl) <= 1e-5 * abs(rl) + 1e-13, (name, k, float(out[k]), rl)
        g = grads[k].double().cpu()
        assert torch.isfinite(g).all(), (name, k)
        for b in range(verts_b.shape[0]):
            top = float(rg[b].abs().max())
            if top == 0:
                assert (g[b] == 0).all(), (name, k, b)
                continue
            err = float((g[b] - rg[b]).abs().max()) / top
            worst = max(worst, err)
            assert err <= 1e-5, (name, k, b, err)
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(MESHES))
def test_regularisers_on_hand_meshes(name, B):
    from smilify_amd import engine

    verts, faces = MESHES[name]
    verts_b = _batch(verts, [2.0 ** -b for b in range(B)])
    topo = _topology(faces, len(verts))
    dv = verts_b.to(DEV)
    full = _poisoned_call(topo, dv, 7)
    worst = _check_reg_against_reference(name, verts_b, faces, full[0], full[1:])
    for terms in range(1, 8):
        out, *grads = engine.mesh_regularisers(topo, dv, terms)
        for k in range(3):
            if terms & (1 << k):  # unchanged by the mask
                assert torch.equal(out[k], full[0][k]) and torch.equal(grads[k], full[1 + k]), (name, terms, k)
            else:
                assert float(out[k]) == 0.0 and grads[k] is None, (name, terms, k)
        out_ng = engine.mesh_regularisers(topo, dv, terms, want_grad=False)
        assert torch.equal(out_ng[0], out) and all(g is None for g in out_ng[1:])
    _report(f"regularisers {name} B={B}", worst_gradient_error_per_mesh=worst)


def test_regulariser_closed_forms():
    from smilify_amd import engine

    def run(name):
        v, f = MESHES[name]
        return engine.mesh_regularisers(_topology(f, len(v)), torch.from_numpy(v)[None].to(DEV), 7)

    out, de, dn, dl = run("triangle")  # Q = 0: the normal term and its gradient are exactly 0
    assert float(out[1]) == 0.0 and (dn == 0).all()
    assert abs(float(out[0]) - 4.0 / 3.0) <= 1e-5 * 4.0 / 3.0  # edges 1, 1, sqrt(2)
    out, *_ = run("tetrahedron")
    assert abs(float(out[0]) - 1.5) <= 1e-5 * 1.5  # three unit edges, three of length sqrt(2)
    out, *_ = run("folded")  # one pair folded by the angle whose sine and cosine are the apex's coordinates
    want = 1.0 - ref.FOLD_COS / np.hypot(ref.FOLD_COS, ref.FOLD_SIN)
    assert abs(want - 0.5) < 1e-7 and abs(float(out[1]) - want) <= 1e-5 * want
    # unreferenced vertices: the Laplacian row is -v_i, and at the origin the gradient is 0 and finite
    v, f = MESHES["isolated"]
    out, de, dn, dl = run("isolated")
    assert (dl[0, 4] == 0).all() and torch.isfinite(dl).all() and (de[0, 4:] == 0).all() and (dn[0, 4:] == 0).all()
    want_5 = torch.from_numpy(v[5]).double() / np.linalg.norm(v[5].astype(np.float64)) / len(v)  # d|-v_5| / dv_5, mean over V
    assert (dl[0, 5].double().cpu() - want_5).abs().max() <= 1e-5 * want_5.abs().max()
    # flat grid: the interior residuals are exactly 0, so the loss is the boundary's alone and no gradient is NaN
    v, f = MESHES["flat_grid_5x5"]
    out, de, dn, dl = run("flat_grid_5x5")
    assert float(out[1]) == 0.0 and (dn == 0).all()
    assert torch.isfinite(dl).all() and torch.isfinite(de).all()


@pytest.mark.parametrize("B", [85, 86, 90])
def test_regulariser_batch_reduce_past_one_block_of_threads(B):
    """k_mesh_reg_reduce strides B * 3 per-mesh sums over 256 threads: B * 3 = 255, 258, 270."""
    verts, faces = MESHES["tetrahedron"]
    verts_b = _batch(verts, [2.0 ** -(b % 4) * (1 + b // 4) for b in range(B)])
    topo = _topology(faces, len(verts))
    out, *grads = _poisoned_call(topo, verts_b.to(DEV), 7)
    _check_reg_against_reference(f"tetrahedron B={B}", verts_b, faces, out, grads)


def test_regularisers_far_from_the_origin():
    """lap_row sums neighbour DIFFERENCES, so a short residual keeps its direction when the coordinates are large: a perturbed
    16 x 16 grid translated by (100, 100, 100), rounded to float32 first; float64 on those inputs is the reference.  Beside the
    kernel's error, that of float32 torch evaluating the reference's formulas.  The normal term is left out of this case: its
    cosines sit near 1 on a nearly flat grid, where 1 - cos cancels in any float32 evaluation and the comparison says nothing
    about the translation."""
    from smilify_amd import engine

    v, faces = ref.tri_grid(16, 16, seed=5, offset=100.0)
    verts_b = torch.from_numpy(v)[None]
    out, de, _, dl = engine.mesh_regularisers(_topology(faces, len(v)), verts_b.to(DEV), 1 | 4)
    for k, got_g, what in ((0, de, "edge"), (2, dl, "laplacian")):
        rl, rg = ref.with_grad(REG_FNS[k], verts_b, faces)
        v32 = verts_b.clone().requires_grad_(True)
        l32 = REG_FNS[k](v32, faces)
        (g32,) = torch.autograd.grad(l32, v32)
        e_loss, y_loss = abs(float(out[k]) - rl), max(abs(float(l32) - rl), U * abs(rl))
        e_grad = float((got_g.double().cpu() - rg).abs().max())
        y_grad = max(float((g32.double() - rg).abs().max()), U * float(rg.abs().max()))
        _report(f"translated grid {what}", kernel_loss_err=e_loss / abs(rl), float32_torch_loss_err=abs(float(l32) - rl) / abs(rl),
                kernel_grad_err=e_grad / float(rg.abs().max()), float32_torch_grad_err=float((g32.double() - rg).abs().max() / rg.abs().max()))
        assert e_loss <= 4 * y_loss, (what, e_loss, y_loss)
        assert e_grad <= 4 * y_grad, (what, e_grad, y_grad)
