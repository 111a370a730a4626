"""GPU tests of the exact point <-> mesh distances (``pytest -m gpu``; ``-s`` prints every measured figure): csrc/point_mesh.hip
against the float64 restatement tests/point_mesh_ref.py, evaluated on the GPU in float64 tensor operations.

The selection bound.  The float32 search decides WHICH face; with d(f) the float64 distance of a point to face f the tests ask, for
every point, d(selected) - min_f d(f) <= c u L: u = 2^-24, L the largest float64 distance from the point to a vertex of the selected
or of the true nearest face, and c = 13 + 40 kappa^2, kappa = (longest edge)^2 / area of the worse of those two faces.  Derivation,
to first order in u, by counting the roundings of point_tri.h as written (vectors: |ap|, |bp|, |cp| <= L, every edge <= e <= 2 L; the
search's power-of-two frame changes no rounding):
  * evaluation, 6.5 u L per face.  r = fma(-w, e2, fma(-v, e1, ap)) with ap = fl(p - v0), e_i = fl(v_i - v0): u (|ap| + v |e1| +
    w |e2|) from the inputs' roundings, u |ap - v e1| and u |r| from the two fma: u (L + 2 L + L + L) = 5 u L on |r|, since v + w <= 1
    and ap - v e1, r are convex combinations of ap, bp, cp.  d^2 = fma(rz, rz, fma(ry, ry, rx rx)) adds 3 u relative on d^2, 1.5 u L on
    d.  Whatever (v, w) the region walk produced, the clamps keep it inside the triangle, so the exact point a + v e1 + w e2 is ON the
    face: the float32 value is never below d(f) by more than this, for the selected face; and it is above by at most this plus the
    parameter error, for the true nearest face.  Twice: 13 u L.
  * parameters, 40 kappa^2 u L.  Each d_i is a three-term fma dot product of vectors with u-relative input errors: at most
    8 u e L.  An edge parameter t = d1 / (d1 - d3) with d1 - d3 = |e1|^2 moves the foot by |e1| dt <= 9 u L, and a vertex / edge
    misclassification needs |d_i| below its error, a foot within 8 u L of the vertex: both below the interior's figure.  Interior:
    vb = d5 d2 - d1 d6 with |d_i| <= e (e + s) for a point whose in-plane offset from the face is s: 2 (2 e^2 8 u e L) + 2 u e^4 <=
    20 u e^3 L for s <= e, three times that on the denominator va + vb + vc = 4 A^2, so dv, dw <= 80 u e^3 L / (4 A^2) and the
    point moves by |e1| dv + |e2| dw <= 40 u L e^4 / A^2 = 40 kappa^2 u L.  An interior / edge misclassification needs |w| <= dw:
    the same displacement.  (s > e: the point is outside the face's prism and a vertex or edge region claims it.)
  * the cap.  The computed point is ON the face wherever its parameters went, so the parameter error of a face is never more than
    its longest edge e: the bound is 13 u L + min(40 kappa^2 u L, e), kappa and e the larger of the two faces'.  It is finite for a
    face of zero area (kappa = inf: there float32 noise decides the signs of va, vb, vc, and the point can land anywhere on the face's
    segment) and no longer grows with kappa for slivers.
kappa^2 is 5.3 for an equilateral and 16 for a right isosceles face (a hull mesh's), so c is 226 and 653 there; it is computed from
the INPUT meshes, per pair of faces, never from the kernel's output, and no point is exempt.  Because this is not the single constant
the issue asks for, the tests also print the largest (d(selected) - min_f d(f)) / (u L) itself, over all pairs and over the pairs with a
zero-area face, beside the largest fraction of the bound; DESIGN.md section 4.20 records them.
"""
import functools
import os

import numpy as np
import pytest
import torch

import point_mesh_cases as PC
import point_mesh_ref as PR
from conftest import GOLDEN, MODEL_FILES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = PR.U
SPLITS = (0, 1, 2, 7)


def _report(name, **figures):
    print(f"\n[point-mesh] {name}: " + ", ".join(f"{k}={v:.4g}" for k, v in figures.items()))


def _tile():
    return PC.TILE


def _meshes(*vf):
    from smilify_amd.mesh3d import Meshes

    return Meshes([torch.as_tensor(v, dtype=torch.float32).to(DEV) for v, _ in vf], [torch.as_tensor(f).long().to(DEV) for _, f in vf])


def _run(meshes, points, lengths=None, by_face=False, splits=0):
    from smilify_amd import engine

    verts = meshes.verts_packed().detach().float().contiguous()
    return engine.point_mesh_distance(verts, meshes.face_tables(), points, lengths, by_face=by_face, splits=splits)


@functools.lru_cache(maxsize=1)
def _atta():
    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    v = torch.from_numpy(d["verts"]).double()
    v = v - v.mean(0)
    v = v / v.abs().max()
    return v.float().to(DEV), torch.from_numpy(d["faces"].astype(np.int64)).to(DEV)


@functools.lru_cache(maxsize=1)
def _sphere_hull():
    """The HullMesh of a voxelised sphere on a 24^3 lattice: faces in lattice order, right isosceles and near it."""
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH

    G = 24
    z, y, x = torch.meshgrid(*(torch.arange(G, dtype=torch.float64) + 0.5,) * 3, indexing="ij")
    occ = (((x - 12.2) ** 2 + (y - 11.9) ** 2 + (z - 12.1) ** 2) < 9.3 ** 2).to(torch.uint8)[None].contiguous().to(DEV)
    mesh = VH.VisualHull(occ, None, None, engine.HullGridSpec(1, (G, G, G), (-1.0, -1.0, -1.0), 2.0 / G)).extract_mesh()
    return mesh.verts.float(), mesh.faces.long()


SEEN = {}  # the largest selection figures of the checks since the last _take_seen()


def _take_seen():
    out = dict(SEEN)
    SEEN.clear()
    return out


def _check(verts, faces, points, dist2, idx, bary, by_face, name, d_all=None):
    """Everything the outputs of one mesh promise, against the restatement; returns the largest fraction of the selection bound.
    verts (V,3), faces (F,3), points (P,3) on the device; dist2 / idx / bary the kernel's rows of this mesh (queries: points, or faces
    when by_face)."""
    v64, p64, faces = verts.double(), points.double(), faces.long()
    d_all = PR.all_pairs(v64, faces, p64) if d_all is None else d_all  # (P,F)
    d_q = d_all.t() if by_face else d_all  # (queries, candidates)
    best2, _ = PR._first_min(d_q, 1)
    none = ~torch.isfinite(best2)
    idx = idx.long()
    assert torch.equal(idx < 0, none), name
    assert torch.isinf(dist2[none]).all() and (bary[none] == 0).all(), name
    assert not torch.isnan(dist2).any() and not torch.isnan(bary).any(), name
    ok = ~none
    if not ok.any():
        return 0.0
    q = torch.nonzero(ok)[:, 0]
    sel = idx[q]
    assert int(sel.max()) < d_q.shape[1], name
    f_sel, p_sel = (q, sel) if by_face else (sel, q)
    # values at the selected pair
    rb, rd2 = PR.dist2_at(v64, faces, p64, f_sel, p_sel)
    far = lambda f, p: (p64[p][:, None, :] - v64[faces[f]]).norm(dim=-1).max(-1).values  # noqa: E731
    # 2 u relative, with the two float64 evaluations' own rounding as the floor (a point ON its face: both values are float64 noise,
    # 2 u of which is nothing).  The residual r = ap - v e1 - w e2 takes four roundings of quantities <= 2 L (two products, two
    # differences; ap, e1, e2 are exact differences of float32 numbers): 4 2^-53 2 L = 8 2^-53 L, in the kernel and in the
    # restatement alike, so the two differ by delta = 16 2^-53 L at most, and their squares by 2 |r| delta + delta^2.  (The
    # parameters' own float64 error moves the point along the face, where d^2 is stationary or, at a clamp, can only grow by the
    # same order.)
    delta = 16 * 2.0 ** -53 * far(f_sel, p_sel)
    tol = 2 * U * rd2 + 2 * rd2.sqrt() * delta + delta ** 2
    assert ((dist2[q].double() - rd2).abs() <= tol).all(), (name, float(((dist2[q].double() - rd2).abs() / tol.clamp(min=1e-300)).max()))
    tri = v64[faces[f_sel]]
    got_c, want_c = (bary[q].double()[..., None] * tri).sum(-2), (rb[..., None] * tri).sum(-2)
    assert ((got_c - want_c).abs() <= 4 * U * v64[torch.isfinite(v64)].abs().max()).all(), name
    assert (bary[q] >= 0).all() and ((bary[q].double().sum(-1) - 1).abs() <= 2 * U).all(), name
    # selection
    true = PR._first_min(d_q, 1)[1][q]
    f_true, p_true = (q, true) if by_face else (true, q)
    d_sel, d_min = d_q[q, sel].sqrt(), best2[q].sqrt()
    L = torch.maximum(far(f_sel, p_sel), far(f_true, p_true))
    kappa, edge = PR.shape_factor(v64, faces), PR.longest_edge(v64, faces)
    worse = torch.maximum(kappa[f_sel], kappa[f_true])
    bound = PR.selection_bound(worse, torch.maximum(edge[f_sel], edge[f_true]), L)
    gap = (d_sel - d_min).clamp(min=0)
    frac = torch.where(gap > 0, gap / bound, torch.zeros_like(gap))
    raw = torch.where(gap > 0, gap / (U * L), torch.zeros_like(gap))
    flat = ~torch.isfinite(worse)
    for key, value in (("gap_over_uL", float(raw.max())), ("gap_over_uL_with_a_zero_area_face", float(raw[flat].max()) if flat.any() else 0.0),
                       ("pairs_with_a_zero_area_face", float(flat.sum()))):
        SEEN[key] = max(SEEN.get(key, 0.0), value) if key != "pairs_with_a_zero_area_face" else SEEN.get(key, 0.0) + value
    assert (gap <= bound).all(), (name, float(frac.max()))
    return float(frac.max())


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def test_hand_cases_exact():
    """Every hand case as a mesh of its own in one batch: face, barycentrics and distance exact (the 1/8 grid is exact in float32)."""
    cases = PC.HAND
    meshes = _meshes(*[(np.asarray(c[1], np.float32), np.asarray([[0, 1, 2]])) for c in cases])
    points = torch.tensor([[c[2]] for c in cases], dtype=torch.float32, device=DEV)
    for by_face in (False, True):
        dist2, idx, bary = _run(meshes, points, by_face=by_face)
        assert (idx == 0).all()
        assert dist2.reshape(-1).tolist() == [c[4] for c in cases]
        assert bary.reshape(-1, 3).tolist() == [[float(x) for x in c[3]] for c in cases]
    cases = PC.DEGENERATE
    meshes = _meshes(*[(np.asarray(c[1], np.float32), np.asarray([[0, 1, 2]])) for c in cases])
    points = torch.tensor([[c[2]] for c in cases], dtype=torch.float32, device=DEV)
    for by_face in (False, True):
        dist2, idx, bary = _run(meshes, points, by_face=by_face)
        tri = torch.tensor([c[1] for c in cases], dtype=torch.float32, device=DEV)
        assert (idx == 0).all() and dist2.reshape(-1).tolist() == [c[4] for c in cases]
        assert (bary.reshape(-1, 3, 1) * tri).sum(1).tolist() == [[float(x) for x in c[3]] for c in cases]
        assert (bary >= 0).all() and (bary.reshape(-1, 3).sum(-1) == 1).all()


@pytest.mark.parametrize("splits", SPLITS)
def test_tie_goes_to_the_smallest_face_whatever_the_split(splits):
    v, f, p, winner = PC.tie_fan(3 * _tile() + 5, (_tile() + 2, _tile() + 3, 2 * _tile() + 4, 3 * _tile() + 4))
    dist2, idx, bary = _run(_meshes((v, f)), torch.from_numpy(p)[None].to(DEV), splits=splits)
    assert int(idx) == winner and float(dist2) == 1.0 and bary.reshape(-1).tolist() == [1.0, 0.0, 0.0]


# ---- the edges of the launch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", sorted({F for F, _ in PC.launch_sizes()}))
def test_launch_edges(F):
    worst = 0.0
    for _, P in [s for s in PC.launch_sizes(_tile()) if s[0] == F]:
        verts, faces = PC.random_mesh(100 + F, 50, F)
        pts = torch.from_numpy(PC.random_cloud(200 + P, P)).to(DEV)
        meshes = _meshes((verts, faces))
        for by_face in (False, True):
            first = None
            for splits in SPLITS:
                out = _run(meshes, pts[None], by_face=by_face, splits=splits)
                if first is None:
                    first = out
                    rows = [o.reshape((-1,) + o.shape[(1 if by_face else 2):]) for o in out]
                    worst = max(worst, _check(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), pts, *rows, by_face,
                                              f"F={F} P={P} by_face={by_face}"))
                else:
                    assert all(torch.equal(a, b) for a, b in zip(first, out)), (F, P, by_face, splits)
    _report(f"launch edges F={F}", worst_fraction_of_selection_bound=worst, **_take_seen())


def test_batch_with_lengths():
    """N = 3 meshes of different sizes, clouds of lengths 257, 0 and 65 in a padded tensor, every split count: equal bits, padded
    points and the empty cloud's faces without a partner."""
    ms, points, lengths = PC.batch(_tile())
    meshes = _meshes(*ms)
    pts, lens = torch.from_numpy(points).to(DEV), torch.from_numpy(lengths).to(DEV)
    foff = np.concatenate([[0], np.cumsum([len(f) for _, f in ms])])
    worst = 0.0
    for by_face in (False, True):
        first = None
        for splits in SPLITS:
            out = _run(meshes, pts, lens, by_face=by_face, splits=splits)
            if first is not None:
                assert all(torch.equal(a, b) for a, b in zip(first, out)), (by_face, splits)
                continue
            first = out
            for n, (v, f) in enumerate(ms):
                rows = [o[foff[n]:foff[n + 1]] for o in out] if by_face else [o[n, :lengths[n]] for o in out]
                worst = max(worst, _check(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), pts[n, :lengths[n]], *rows, by_face,
                                          f"batch mesh {n} by_face={by_face}"))
                if not by_face:
                    assert (out[1][n, lengths[n]:] == -1).all() and torch.isinf(out[0][n, lengths[n]:]).all()
                    assert (out[2][n, lengths[n]:] == 0).all()
        if by_face:
            assert (first[1][foff[1]:foff[2]] == -1).all() and torch.isinf(first[0][foff[1]:foff[2]]).all()
    _report("batch with lengths", worst_fraction_of_selection_bound=worst, **_take_seen())


# ---- selection and values on real surfaces ----------------------------------------------------------------------------------------
def _surface_cloud(verts, faces, seed, n_on=1500, n_around=1500):
    from smilify_amd import fit3d

    meshes = _meshes((verts, faces))
    on, _ = fit3d.sample_points_with_faces(meshes, n_on, seed=seed)
    g = torch.Generator().manual_seed(seed)
    around = on[0, torch.randint(0, n_on, (n_around,), generator=g).to(DEV)] \
        + (0.3 * torch.randn(n_around, 3, generator=g) * torch.rand(n_around, 1, generator=g) ** 3).to(DEV)
    return meshes, torch.cat([on[0], around.float()]).contiguous()


@pytest.mark.parametrize("which", ["atta", "hull"])
def test_selection_and_values_on_surfaces(which):
    """Clouds on and around the atta worker's mesh and a carved sphere's hull mesh, both directions: the selection bound of this file's
    docstring for every point / face, and the values at the selected pair."""
    verts, faces = _atta() if which == "atta" else _sphere_hull()
    meshes, pts = _surface_cloud(verts, faces, 31 if which == "atta" else 32)
    d_all = PR.all_pairs(verts.double(), faces, pts.double())
    kappa = PR.shape_factor(verts, faces)
    for by_face in (False, True):
        out = _run(meshes, pts[None], by_face=by_face)
        rows = [o.reshape((-1,) + o.shape[(1 if by_face else 2):]) for o in out]
        frac = _check(verts, faces, pts, *rows, by_face, f"{which} by_face={by_face}", d_all)
        ties = float((d_all.t() if by_face else d_all).sort(1).values[:, :2].diff(dim=1).eq(0).double().mean())
        _report(f"selection {which} {'faces -> points' if by_face else 'points -> faces'} F={len(faces)} P={len(pts)}",
                worst_fraction_of_selection_bound=frac, **_take_seen(), kappa_median=float(kappa.median()), kappa_max=float(kappa.max()),
                queries_with_a_float64_tie=ties)


# ---- degenerate and non-finite input -------------------------------------------------------------------------------------------------
def test_degenerate_faces_and_non_finite_input():
    from smilify_amd import fit3d

    verts, faces = PC.random_mesh(41, 60, 2 * _tile() + 9, degenerate=True)
    pts = PC.random_cloud(42, 300)
    v, f, p = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), torch.from_numpy(pts).to(DEV)
    for by_face in (False, True):
        out = _run(_meshes((verts, faces)), p[None], by_face=by_face)
        rows = [o.reshape((-1,) + o.shape[(1 if by_face else 2):]) for o in out]
        assert torch.isfinite(rows[0]).all()
        frac = _check(v, f, p, *rows, by_face, f"degenerate by_face={by_face}")
        _report(f"degenerate soup by_face={by_face}", worst_fraction_of_selection_bound=frac, **_take_seen())
    # a NaN and an inf in two points, a NaN and an inf in two vertices
    bad_v, bad_p = v.clone(), p.clone()
    bad_v[int(f[5, 1]), 2] = float("nan")
    bad_v[int(f[70, 0]), 0] = float("inf")
    bad_p[3, 1] = float("nan")
    bad_p[200, 0] = float("-inf")
    poisoned = ~torch.isfinite(bad_v[f]).all(-1).all(-1)
    assert 2 <= int(poisoned.sum()) < len(f)
    meshes = _meshes((bad_v.cpu().numpy(), faces))
    for by_face in (False, True):
        out = _run(meshes, bad_p[None], by_face=by_face)
        dist2, idx, bary = [o.reshape((-1,) + o.shape[(1 if by_face else 2):]) for o in out]
        _check(bad_v, f, bad_p, dist2, idx, bary, by_face, f"non-finite by_face={by_face}")
        _take_seen()
        if by_face:
            assert (idx[poisoned] == -1).all() and (idx[~poisoned] >= 0).all() and not torch.isin(idx, torch.tensor([3, 200], device=DEV)).any()
        else:
            assert idx[3] == -1 and idx[200] == -1 and (idx[[0, 1, 2, 4, 199, 201]] >= 0).all() and not poisoned[idx[idx >= 0].long()].any()
    # gradients: zero for the two points, finite everywhere
    vv, pp = bad_v.clone().requires_grad_(True), bad_p[None].clone().requires_grad_(True)
    from smilify_amd.mesh3d import Meshes

    d, face = fit3d.point_face_distance(Meshes([vv], [f]), pp)
    torch.where(face >= 0, d, torch.zeros_like(d)).sum().backward()
    assert torch.isfinite(vv.grad).all() and torch.isfinite(pp.grad).all()
    assert (pp.grad[0, [3, 200]] == 0).all() and (pp.grad[0, :3] != 0).any()


# ---- gradients -------------------------------------------------------------------------------------------------------------------------
YARDSTICK_ASSERTED = (0, 10, 20)  # as the chamfer sweep: further down float32 torch, the yardstick itself, underflows; measured there


def _scaled_batch(k):
    ms, points, lengths = PC.batch(_tile())
    s = np.float32(2.0 ** -k)
    return [(v * s, f) for v, f in ms], points * s, lengths


def _backward(ms, points, lengths, by_face, g):
    from smilify_amd import engine

    meshes = _meshes(*ms)
    verts = meshes.verts_packed().contiguous()
    pts, lens = torch.from_numpy(points).to(DEV), torch.from_numpy(lengths).to(DEV)
    _, idx, _ = engine.point_mesh_distance(verts, meshes.face_tables(), pts, lens, by_face=by_face)
    d_points, d_verts = engine.point_mesh_backward(verts, meshes.face_tables(), pts, lens, idx, g, by_face=by_face)
    return idx, d_points, d_verts


@pytest.mark.parametrize("by_face", [False, True], ids=["points->faces", "faces->points"])
def test_gradients_and_scale_sweep(by_face):
    """The gradient of sum_r g_r dist2_r against float64 autograd of the restatement at the kernel's indices, with the project's
    chamfer yardstick (test_gpu_mesh3d_kernels.py): per mesh at most 4 x the error of float32 torch on the same restatement at the
    same indices, floored at half an ulp of the mesh's largest gradient (asserted at 2^0, 2^-10 and 2^-20, measured further), and
    exactly 0 where the reference is 0.  Scaling every input by 2^-k, k up to 50, changes no index and scales every gradient by
    exactly 2^-k (a constant fixed-point unit fails this)."""
    ms0, _, lengths = PC.batch(_tile())
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in ms0])])
    foff = np.concatenate([[0], np.cumsum([len(f) for _, f in ms0])])
    n_rec = int(foff[-1]) if by_face else 3 * 257
    g = torch.from_numpy(np.random.default_rng(50).standard_normal(n_rec).astype(np.float32)).to(DEV)
    g = g if by_face else g.reshape(3, 257)
    base = None
    for k in (0, 10, 20, 30, 40, 50):
        ms, points, _ = _scaled_batch(k)
        idx, d_points, d_verts = _backward(ms, points, lengths, by_face, g)
        worst = 0.0
        for n, (v, f) in enumerate(ms):
            ln = int(lengths[n])
            rec = idx[foff[n]:foff[n + 1]] if by_face else idx[n, :ln]
            gn = g[foff[n]:foff[n + 1]] if by_face else g[n, :ln]
            keep = torch.nonzero(rec >= 0)[:, 0]
            f_idx, p_idx = (keep, rec[keep].long()) if by_face else (rec[keep].long(), keep)
            grads = {}
            for dtype in (torch.float64, torch.float32):
                vr = torch.from_numpy(v).to(DEV, dtype).requires_grad_(True)
                pr = torch.from_numpy(points[n, :ln]).to(DEV, dtype).requires_grad_(True)
                if len(keep):
                    _, d2 = PR.dist2_at(vr, torch.from_numpy(f).to(DEV), pr, f_idx, p_idx)
                    grads[dtype] = torch.autograd.grad((gn[keep].to(dtype) * d2).sum(), (pr, vr))
                else:
                    grads[dtype] = (torch.zeros_like(pr), torch.zeros_like(vr))
            for got, want, yard in zip((d_points[n, :ln], d_verts[voff[n]:voff[n + 1]]), grads[torch.float64], grads[torch.float32]):
                if not want.numel():
                    continue
                e_k = float((got.double() - want).abs().max())
                e_y = max(float((yard.double() - want).abs().max()), U * float(want.abs().max()))
                if k in YARDSTICK_ASSERTED:
                    assert e_k <= 4 * e_y, (k, n, e_k, e_y)
                assert (got[want == 0] == 0).all(), (k, n)
                worst = max(worst, e_k / e_y) if e_y > 0 else worst
            assert (d_points[n, ln:] == 0).all()
        _report(f"gradient {'faces -> points' if by_face else 'points -> faces'} 2^-{k}", worst_error_over_yardstick=worst)
        if base is None:
            base = (idx, d_points, d_verts)
        else:
            assert torch.equal(idx, base[0]), k
            assert torch.equal(d_points * 2.0 ** k, base[1]) and torch.equal(d_verts * 2.0 ** k, base[2]), k


def test_two_calls_and_permuted_points():
    """Two calls give equal bits; permuting the points permutes the point outputs and leaves the vertex gradients bit-identical."""
    ms, points, _ = PC.batch(_tile())
    lengths = np.asarray([257, 257, 257], np.int32)
    g = torch.from_numpy(np.random.default_rng(51).standard_normal((3, 257)).astype(np.float32)).to(DEV)
    meshes = _meshes(*ms)
    pts = torch.from_numpy(points).to(DEV)
    fwd = _run(meshes, pts)
    assert all(torch.equal(a, b) for a, b in zip(fwd, _run(meshes, pts)))
    a, b = _backward(ms, points, lengths, False, g), _backward(ms, points, lengths, False, g)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(52)).to(DEV)
    fwd_p = _run(meshes, pts[:, perm].contiguous())
    assert all(torch.equal(x[:, perm], y) for x, y in zip(fwd, fwd_p))
    c = _backward(ms, points[:, perm.cpu().numpy()], lengths, False, g[:, perm].contiguous())
    assert torch.equal(a[1][:, perm], c[1]) and torch.equal(a[2], c[2])
    # faces -> points: the point index follows the permutation, the vertex gradients keep their bits
    gf = torch.from_numpy(np.random.default_rng(53).standard_normal(meshes.face_tables().n_faces).astype(np.float32)).to(DEV)
    a, c = _backward(ms, points, lengths, True, gf), _backward(ms, points[:, perm.cpu().numpy()], lengths, True, gf)
    assert torch.equal(a[2], c[2]) and torch.equal(a[1][:, perm], c[1])


# ---- the loss, the optimiser and the Stage --------------------------------------------------------------------------------------------
def test_loss_against_restatement_and_zero_on_own_samples():
    """point_mesh_face_distance on the seeded batch against the restatement (1e-6 relative); closest_points agrees with it; and a
    mesh against points sampled on itself: the point -> face mean is below the square of the selection bound at its largest over the
    points (the face -> point mean is the distance to the nearest SAMPLE and does not vanish)."""
    from smilify_amd import fit3d, mesh3d

    ms, points, lengths = PC.batch(_tile())
    meshes = _meshes(*ms)
    pts, lens = torch.from_numpy(points).to(DEV), torch.from_numpy(lengths).to(DEV)
    got = float(fit3d.point_mesh_face_distance(meshes, pts, lens))
    want = PR.loss(ms, [points[n, :lengths[n]] for n in range(3)])
    _report("loss", kernel=got, restatement=want, relative_error=abs(got - want) / want)
    assert abs(got - want) <= 1e-6 * want
    cp = mesh3d.closest_points(meshes, pts, lens)
    d2, face = fit3d.point_face_distance(meshes, pts, lens)
    assert torch.equal(cp.dist2, d2) and torch.equal(cp.face, face) and cp.face.dtype == torch.int64
    ok = face >= 0
    assert (((cp.points - pts) ** 2).sum(-1)[ok] - d2[ok]).abs().max() <= 1e-5 * d2[ok].max()
    verts, faces = _atta()
    own = _meshes((verts, faces))
    on, _ = fit3d.sample_points_with_faces(own, 2000, seed=33)
    d2, face = fit3d.point_face_distance(own, on)
    L = (on[0, :, None, :].double() - verts.double()[faces[face[0]]]).norm(dim=-1).max(-1).values
    bound = float(PR.selection_bound(PR.shape_factor(verts, faces)[face[0]], PR.longest_edge(verts, faces)[face[0]], L).max()) ** 2
    _report("own samples", mean_dist2=float(d2.mean()), bound=bound)
    assert float(d2.mean()) < bound


def test_adam_recovers_a_translation():
    """A copy of the atta mesh moved by a tenth of its extent is brought back by torch Adam on point_face_distance: the loss falls
    below 1e-4 of its start within 100 steps."""
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    verts, faces = _atta()
    on, _ = fit3d.sample_points_with_faces(_meshes((verts, faces)), 2000, seed=34)
    extent = float((verts.max(0).values - verts.min(0).values).max())
    moved = verts + 0.1 * extent * torch.tensor([0.6, -0.48, 0.64], device=DEV)
    t = torch.zeros(3, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([t], lr=0.01)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        d2, _ = fit3d.point_face_distance(Meshes([moved + t], [faces]), on)
        loss = d2.mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    _report("translation", start=float(losses[0]), lowest=float(losses.min()), last=float(losses[-1]))
    assert float(losses.min()) < 1e-4 * float(losses[0])


def test_stage_surface_term_and_default_path():
    from smilify_amd import fit3d
    from smilify_amd.mesh3d import Meshes

    def problem():
        torch.manual_seed(0)
        model = fit3d.SMAL3DFitter(batch_size=1, device=DEV, model_path=MODEL_FILES["stick"])
        with torch.no_grad():
            tv = model() + torch.tensor([0.05, -0.03, 0.02], device=DEV)
        return model, Meshes([tv[0]], [model.faces[0]])

    model, target = problem()
    stage = fit3d.Stage(30, "init", model, target, lr=0.005,
                        loss_weights=dict(w_chamfer=0, w_edge=0, w_normal=0, w_laplacian=0, w_surface=1))
    stage.run()
    s = torch.stack(stage.loss_components_to_plot["surface"]).cpu()
    _report("stage surface", first=float(s[0]), last=float(s[-1]))
    assert list(stage.loss_components_to_plot) == ["surface"] and torch.isfinite(s).all() and float(s[-1]) < float(s[0])
    # without the key: the losses of the iteration are those of the terms evaluated here, bit for bit, on the same seed
    model, target = problem()
    stage = fit3d.Stage(1, "init", model, target, lr=0.005)
    assert "w_surface" not in stage.loss_weights
    torch.manual_seed(7)
    loss, comps = stage.forward(stage.src_mesh)
    torch.manual_seed(7)
    tv = fit3d.sample_points_from_meshes(target, 3000)
    chamfer, _ = fit3d.chamfer_distance(tv, stage.src_mesh.verts_padded())
    reg = fit3d.mesh_regularisers(stage.src_mesh, True, True, True)
    w = fit3d.default_weights
    want = 0 + w["w_chamfer"] * chamfer
    for name, r in zip(("edge", "normal", "laplacian"), reg.unbind(0)):
        want = want + w[f"w_{name}"] * r
    assert sorted(comps) == ["chamfer", "edge", "laplacian", "normal"] and torch.equal(loss, want)
    assert torch.equal(comps["chamfer"], chamfer) and torch.equal(stage.last_target_samples, tv)


def test_unusable_coordinates_and_hand_made_records():
    """A finite coordinate above 3e38 makes a point "none" whatever the frame does to it (with data of 2^66 the frame scales DOWN and
    the point would get a distance), and the backward ignores a hand-made record that names a face with a NaN vertex or such a
    point: finite gradients, nothing added."""
    from smilify_amd import engine

    s = np.float32(2.0 ** 66)
    verts, faces = PC.random_mesh(61, 30, 70)
    pts = PC.random_cloud(62, 90)
    pts_big = pts * s
    pts_big[17, 1] = np.float32(3.3e38)
    meshes = _meshes((verts * s, faces))
    _, idx, _ = _run(meshes, torch.from_numpy(pts_big)[None].to(DEV))
    assert int(idx[0, 17]) == -1 and (idx[0, :17] >= 0).all() and (idx[0, 18:] >= 0).all()
    _, pidx, _ = _run(meshes, torch.from_numpy(pts_big)[None].to(DEV), by_face=True)
    assert (pidx >= 0).all() and (pidx != 17).all()
    # records by hand: face 5 has a NaN vertex, point 17 a coordinate above 3e38, face 70 does not exist
    bad_v = verts.copy()
    bad_v[faces[5, 2], 0] = np.nan
    bad_p = pts.copy()
    bad_p[17, 1] = np.float32(-3.3e38)
    meshes = _meshes((bad_v, faces))
    v, p = meshes.verts_packed().contiguous(), torch.from_numpy(bad_p)[None].to(DEV)
    _, idx, _ = engine.point_mesh_distance(v, meshes.face_tables(), p)
    forged = idx.clone()
    forged[0, 3], forged[0, 17], forged[0, 20] = 5, 9, 70
    g = torch.ones(1, 90, device=DEV)
    dp, dv = engine.point_mesh_backward(v, meshes.face_tables(), p, None, forged, g)
    assert torch.isfinite(dp).all() and torch.isfinite(dv).all() and (dp[0, [3, 17, 20]] == 0).all()
    keep = idx.clone()
    keep[0, 3], keep[0, 20] = -1, -1
    dp2, dv2 = engine.point_mesh_backward(v, meshes.face_tables(), p, None, keep, g)
    assert torch.equal(dp, dp2) and torch.equal(dv, dv2)
