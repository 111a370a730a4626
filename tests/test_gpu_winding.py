"""GPU tests of the winding numbers and what is built on them (``pytest -m gpu``; ``-s`` prints every measured figure): k_pm_winding of
csrc/point_mesh.hip against the restatement tests/winding_ref.py in float64, with the float32 restatement as the yardstick;
``mesh3d.winding_number / contains / signed_distance`` and ``fit3d.point_mesh_signed_distance / containment_loss / penetration_loss``.

Decisions: for every point whose float64 distance to the surface is at least 2^-14 E (E the largest |coordinate| of mesh and cloud),
``w > 0.5`` equals the float64 restatement's; no such point is exempt.  The cases hold no point with a float64 |w - 0.5| < 0.05
(tests/test_winding_cpu.py asserts it), so the side of every point is a fact about the mesh.  Values: the largest |w - w64| over a
case set is at most 4 x the largest error of the float32 restatement against the float64 one over the same set, floored at 4 u,
u = 2^-24 (the output's own rounding at |w| ~ 1 with a margin).
"""
import functools

import numpy as np
import pytest
import torch

import point_mesh_cases as PC
import point_mesh_ref as PR
import winding_cases as WC
import winding_ref as WR
from conftest import MODEL_FILES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = WR.U
SPLITS = (1, 2, 3, 7, 0)
HAND_EPS = 2.0 ** -22  # tests/test_winding_cpu.py's float32 figure: a few roundings of values <= 1


def _report(name, **figures):
    print(f"\n[winding] {name}: " + ", ".join(f"{k}={v:.4g}" for k, v in figures.items()))


def _meshes(*vf):
    from smilify_amd.mesh3d import Meshes

    return Meshes([torch.as_tensor(np.asarray(v), dtype=torch.float32).to(DEV) for v, _ in vf],
                  [torch.as_tensor(np.asarray(f)).long().reshape(-1, 3).to(DEV) for _, f in vf])


def _dev(x):
    return torch.as_tensor(np.asarray(x, np.float32)).to(DEV)


def _run(meshes, points, lengths=None, splits=0):
    from smilify_amd import engine

    verts = meshes.verts_packed().detach().float().contiguous()
    return engine.point_mesh_winding(verts, meshes.face_tables(), points, lengths, splits=splits)


def _same(a, b):
    """Equal bits, NaN included."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _one(v, f, p):
    """The kernel's winding numbers (P,) of one mesh, as float64 numpy."""
    return _run(_meshes((v, f)), _dev(p).reshape(1, -1, 3)).double().cpu().numpy()[0]


def _yardstick(v, f, p):
    """(w64, the float32 restatement's largest error) of one mesh on the device."""
    w64 = WR.winding(v, f, p, np.float64, DEV)
    w32 = WR.winding(v, f, p, np.float32, DEV)
    ok = np.isfinite(w64)
    return w64, float(np.abs(w32 - w64)[ok].max()) if ok.any() else 0.0


def _check_values(name, got, w64, yard):
    ok = np.isfinite(w64)
    assert np.array_equal(np.isnan(got), ~ok), name
    err = float(np.abs(got - w64)[ok].max()) if ok.any() else 0.0
    tol = max(4.0 * yard, 4.0 * U)
    _report(name, kernel_error=err, float32_restatement_error=yard, allowed=tol, fraction_of_yardstick=err / max(yard, U))
    assert err <= tol, (name, err, yard)
    return err


# ---- hand cases -----------------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    octant = np.asarray(WC.OCTANT, np.float32)
    assert abs(_one(octant, [[0, 1, 2]], [[0, 0, 0]])[0] - 0.125) <= HAND_EPS
    assert abs(_one(octant, [[2, 1, 0]], [[0, 0, 0]])[0] + 0.125) <= HAND_EPS
    inside, outside = [[0, 0, 0], [0.25, -0.5, 0.75]], [[3, 0.25, 0.125], [-1.5, 1.5, 1.5]]
    v, f = WC.cube()
    for t in f:
        assert abs(_one(v, [t], [[0, 0, 0]])[0] - 1.0 / 12.0) <= HAND_EPS
    assert np.abs(_one(v, f, inside) - 1.0).max() <= 12 * HAND_EPS and np.abs(_one(v, f, outside)).max() <= 12 * HAND_EPS
    assert np.abs(_one(*WC.cube(flip=True), inside) + 1.0).max() <= 12 * HAND_EPS
    assert np.abs(_one(*WC.nested_cubes(), [[0, 0, 0], [0.25, 0.125, -0.25]]) - 2.0).max() <= 24 * HAND_EPS
    assert abs(_one(*WC.nested_cubes(), [[0.75, 0, 0]])[0] - 1.0) <= 24 * HAND_EPS
    assert abs(_one(*WC.cube(top=False), [[0, 0, 0]])[0] - 5.0 / 6.0) <= 12 * HAND_EPS
    # det == 0 adds exactly 0
    tri = np.asarray(PC.TRI, np.float32)
    flat = [[0.25, 0.25, 0.0], [2.0, 3.0, 0.0], [-1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.0, 0.0]]
    got = _one(tri, [[0, 1, 2]], flat)
    assert (got == 0).all() and not np.signbit(got).any()
    for _, t, p, _, _ in PC.DEGENERATE:
        assert (_one(np.asarray(t, np.float32), [[0, 1, 2]], [p, [0.3, -0.7, 0.2]]) == 0).all()
    w = _one(v, f, v)  # on the vertices of the cube: finite, an octant each
    assert np.isfinite(w).all() and np.abs(w - 0.125).max() <= 12 * HAND_EPS


# ---- the edges of the launch and equal bits ------------------------------------------------------------------------------------------
def _equal_bits_everywhere(ms, points, lengths, name):
    """Every split count, a second call, a permutation of the faces and the inputs scaled by 2^20 and 2^-20: the same bits."""
    pts = _dev(points)
    lens = None if lengths is None else torch.as_tensor(lengths).to(DEV)
    meshes = _meshes(*ms)
    base = _run(meshes, pts, lens, splits=SPLITS[0])
    for splits in SPLITS[1:]:
        assert _same(base, _run(meshes, pts, lens, splits=splits)), (name, splits)
    assert _same(base, _run(meshes, pts, lens, splits=SPLITS[0])), name
    rng = np.random.default_rng(5)
    assert _same(base, _run(_meshes(*[(v, np.asarray(f)[rng.permutation(len(f))]) for v, f in ms]), pts, lens)), name
    for s in (2.0 ** 20, 2.0 ** -20):
        scaled = _meshes(*[(np.asarray(v, np.float32) * np.float32(s), f) for v, f in ms])
        assert _same(base, _run(scaled, pts * s, lens)), (name, s)
    return base


@pytest.mark.parametrize("F", sorted({F for F, _ in PC.launch_sizes()}))
def test_launch_edges(F):
    for _, P in [s for s in PC.launch_sizes(PC.TILE) if s[0] == F]:
        verts, faces = PC.random_mesh(100 + F, 50, F)
        pts = PC.random_cloud(200 + P, P)
        got = _equal_bits_everywhere([(verts, faces)], pts[None], None, f"F={F} P={P}")
        w64, yard = _yardstick(verts, faces, pts)
        _check_values(f"launch edges F={F} P={P}", got[0].double().cpu().numpy(), w64, yard)


def test_batch_with_lengths():
    from smilify_amd import mesh3d

    ms, points, lengths = PC.batch(PC.TILE)
    got = _equal_bits_everywhere(ms, points, lengths, "batch")
    inside = mesh3d.contains(_meshes(*ms), _dev(points), torch.as_tensor(lengths).to(DEV))
    assert inside.dtype == torch.bool and tuple(inside.shape) == (3, 257)
    for n, (v, f) in enumerate(ms):
        ln = int(lengths[n])
        assert torch.isnan(got[n, ln:]).all() and not inside[n, ln:].any()
        if ln:
            assert _same(got[n, :ln], _run(_meshes((v, f)), _dev(points[n, :ln])[None])[0]), n  # the mesh alone: the same frame and bits
            w64, yard = _yardstick(v, f, points[n, :ln])
            _check_values(f"batch mesh {n}", got[n, :ln].double().cpu().numpy(), w64, yard)
            assert torch.equal(inside[n, :ln], got[n, :ln] > 0.5)


def test_unusable_input_and_empty_meshes():
    from smilify_amd import mesh3d

    verts, faces = WC.soup()
    pts = PC.random_cloud(6, 300)
    base = _run(_meshes((verts, faces)), _dev(pts)[None])[0]
    assert torch.isfinite(base).all()
    # non-finite and unusable points: NaN, and nothing else changes
    bad_p = pts.copy()
    bad_p[3, 1], bad_p[200, 0], bad_p[17, 2] = np.nan, -np.inf, np.float32(3.3e38)
    got = _run(_meshes((verts, faces)), _dev(bad_p)[None])[0]
    keep = torch.ones(300, dtype=torch.bool, device=DEV)
    keep[[3, 200, 17]] = False
    assert torch.isnan(got[~keep]).all() and _same(got[keep], base[keep])
    assert not mesh3d.contains(_meshes((verts, faces)), _dev(bad_p)[None])[0, ~keep].any()
    # a face with a NaN vertex of its own, and one with an index out of range, add nothing: the bits of the mesh without them
    drop = [5, 140]
    v2 = np.concatenate([verts, np.asarray([[0.5, np.nan, 0.25]], np.float32)])
    f2 = faces.copy()
    f2[drop[0], 1] = len(verts)  # the NaN vertex
    f2[drop[1], 2] = len(v2) + 7
    assert len(bin(len(faces))) == len(bin(len(faces) - 2))  # (the same integer unit)
    without = _run(_meshes((verts, np.delete(faces, drop, 0))), _dev(pts)[None])[0]
    assert _same(_run(_meshes((v2, f2)), _dev(pts)[None])[0], without)
    # a mesh without faces in a batch: 0
    both = _meshes((verts, faces), (verts[:4], np.zeros((0, 3), np.int64)))
    got = _run(both, _dev(np.stack([pts, pts])))
    assert _same(got[0], base) and (got[1] == 0).all()


# ---- decisions and values on the meshes the sign must survive ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    return WC.case(name, DEV)


@pytest.mark.parametrize("name", WC.NAMES)
def test_decisions_values_and_signed_distance(name):
    from smilify_amd import mesh3d

    v, f, p = _case(name)
    meshes, pts = _meshes((v, f)), _dev(p)[None]
    w64, yard = _yardstick(v, f, p)
    assert float(np.abs(w64 - 0.5).min()) >= WC.BAND
    got = mesh3d.winding_number(meshes, pts)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, len(p)) and _same(got, _run(meshes, pts))
    w = got[0].double().cpu().numpy()
    d64 = PR.point_face(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(p).to(DEV))[0].sqrt().cpu().numpy()
    decided = d64 >= WC.DECIDED_FROM * WC.extent(v, p)
    wrong = decided & ((w > 0.5) != (w64 > 0.5))
    _report(f"decisions {name}", faces=len(f), points=len(p), decided=int(decided.sum()), wrong=int(wrong.sum()),
            differ_below=int((~decided & ((w > 0.5) != (w64 > 0.5))).sum()))
    assert not wrong.any(), (name, np.nonzero(wrong)[0].tolist())
    _check_values(f"values {name}", w, w64, yard)
    # the signed distance: closest_points with contains' sign
    for oriented in (True, False):
        sd = mesh3d.signed_distance(meshes, pts, oriented=oriented)
        cp = mesh3d.closest_points(meshes, pts)
        inside = mesh3d.contains(meshes, pts, oriented=oriented)
        assert torch.equal(inside, (got if oriented else got.abs()) > 0.5)
        assert all(torch.equal(a, b) for a, b in zip(sd[1:5], cp)) and _same(sd.winding, got)
        assert torch.equal(sd.sdist, torch.where(inside, -cp.dist2.sqrt(), cp.dist2.sqrt()))
    assert inside.any() and not inside.all()


@pytest.mark.parametrize("name", ["icosphere", "atta", "hull"])
def test_surface_points(name):
    """Points on the faces and 2^-30 E off them: the winding number is finite and the signed distance is the unsigned one with a sign."""
    from smilify_amd import mesh3d

    v, f = next(c[1] for c in WC.mesh_cases() if c[0] == name)
    meshes, pts = _meshes((v, f)), _dev(WC.surface_cloud(v, f, 91))[None]
    sd = mesh3d.signed_distance(meshes, pts)
    cp = mesh3d.closest_points(meshes, pts)
    assert torch.isfinite(sd.winding).all()
    assert torch.equal(sd.dist2, cp.dist2) and torch.equal(sd.sdist.abs(), cp.dist2.sqrt())


def test_hull_mesh_contains_its_voxels():
    """The small carve: the unrelaxed mesh contains exactly the occupied voxel centres; after taubin_steps(4) the same holds for every
    voxel whose 26 neighbours share its occupancy (relaxation keeps every vertex in its own cube)."""
    from smilify_amd import engine, mesh3d
    from smilify_amd import visual_hull as VH

    occ = WC.hull_occupancy()
    G = WC.HULL_G
    hull = VH.VisualHull(torch.from_numpy(occ).to(DEV), None, None, engine.HullGridSpec(1, (G, G, G), WC.HULL_ORIGIN, WC.HULL_VOXEL))
    centres = _dev(WC.hull_centres())[None]
    want = torch.from_numpy(occ.reshape(-1) != 0).to(DEV)
    same = torch.from_numpy(WC.hull_uniform_neighbourhood()).to(DEV)
    _report("hull consistency", voxels=len(want), share_left_out_after_relaxation=1.0 - float(same.double().mean()))
    assert 1.0 - float(same.double().mean()) < 0.5
    for steps, which in (((), torch.ones_like(same)), (VH.taubin_steps(4), same)):
        mesh = hull.extract_mesh(relax_steps=steps, return_normals=False)
        inside = mesh3d.contains(_meshes((mesh.verts.float().cpu().numpy(), mesh.faces.cpu().numpy())), centres)[0]
        assert torch.equal(inside[which], want[which]), len(steps)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------------
def _gradient_batch():
    """Two closed meshes with clouds half inside: an icosphere of 320 faces and a cube; lengths (257, 65); a point on a vertex
    (dist2 == 0) and a non-finite point (index -1) in the first cloud."""
    ms = [WC.icosphere(2), WC.cube(-0.5, 0.75)]
    points = np.stack([PC.random_cloud(95, 257, 0.6), PC.random_cloud(96, 257, 0.5)])
    points[0, 9] = ms[0][0][40]
    points[0, 11, 1] = np.nan
    return ms, points, np.asarray([257, 65], np.int32)


def _reference_loss(kind, ms, points, lengths, face, inside, g, dtype):
    """The loss ``kind`` at the kernel's faces and sides as torch operations in ``dtype``: (loss, [(points_n, verts_n)] leaves)."""
    total, leaves = 0, []
    for n, (v, f) in enumerate(ms):
        ln = int(lengths[n])
        vr = torch.from_numpy(np.asarray(v, np.float32)).to(DEV, dtype).requires_grad_(True)
        pr = torch.from_numpy(points[n, :ln]).to(DEV, dtype).requires_grad_(True)
        leaves.append((pr, vr))
        ok = face[n, :ln] >= 0
        keep = torch.nonzero(ok)[:, 0]
        _, d2 = PR.dist2_at(vr, torch.from_numpy(np.asarray(f)).to(DEV), pr, face[n, :ln][keep], keep)
        side = inside[n, :ln][keep]
        if kind == "sdist":
            live = d2 > 0
            d = torch.where(live, d2, torch.ones_like(d2)).sqrt()
            sign = torch.where(side, -torch.ones_like(d), torch.ones_like(d))
            total = total + (g[n, :ln][keep].to(dtype) * sign * torch.where(live, d, torch.zeros_like(d))).sum()
        else:
            counted = side if kind == "penetration" else ~side
            total = total + torch.where(counted, d2, torch.zeros_like(d2)).sum() / ln / len(ms)
    return total, leaves


@pytest.mark.parametrize("kind", ["sdist", "containment", "penetration"])
def test_gradients(kind):
    """Against float64 autograd of the restatement at the kernel's faces and sides, with tests/test_gpu_point_mesh.py's bound: per mesh
    at most 4 x the error of float32 torch on the same restatement, floored at half an ulp of the largest gradient, and exactly 0
    on the surface, without a face, and on the side the loss ignores."""
    from smilify_amd import fit3d, mesh3d

    ms, points, lengths = _gradient_batch()
    meshes = _meshes(*ms)
    pts, lens = _dev(points).requires_grad_(True), torch.as_tensor(lengths).to(DEV)
    verts = meshes.verts_packed().clone().requires_grad_(True)
    live = meshes.offset_verts(verts - meshes.verts_packed())
    inside = mesh3d.contains(meshes, pts.detach(), lens)
    g = torch.from_numpy(np.random.default_rng(97).standard_normal((2, 257)).astype(np.float32)).to(DEV)
    if kind == "sdist":
        sdist, face = fit3d.point_mesh_signed_distance(live, pts, lens)
        cp = mesh3d.closest_points(meshes, pts.detach(), lens)
        assert torch.equal(face, cp.face) and torch.equal(sdist, torch.where(inside, -cp.dist2.sqrt(), cp.dist2.sqrt()))
        assert int(face[0, 11]) == -1 and float(cp.dist2[0, 9]) == 0.0 and torch.isinf(sdist[0, 11]) and (face[1, 65:] == -1).all()
        loss = (g * torch.where(face >= 0, sdist, torch.zeros_like(sdist))).sum()
    else:
        fn = fit3d.containment_loss if kind == "containment" else fit3d.penetration_loss
        loss = fn(live, pts, lens)
        face = mesh3d.closest_points(meshes, pts.detach(), lens).face
    dist2 = mesh3d.closest_points(meshes, pts.detach(), lens).dist2
    d_points, d_verts = torch.autograd.grad(loss, (pts, verts))
    want64, leaves64 = _reference_loss(kind, ms, points, lengths, face, inside, g, torch.float64)
    want32, leaves32 = _reference_loss(kind, ms, points, lengths, face, inside, g, torch.float32)
    assert abs(float(loss.detach()) - float(want64.detach())) <= 1e-5 * max(abs(float(want64.detach())), 1.0)
    g64 = torch.autograd.grad(want64, [t for pair in leaves64 for t in pair])
    g32 = torch.autograd.grad(want32, [t for pair in leaves32 for t in pair])
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in ms])])
    worst = 0.0
    for n in range(len(ms)):
        ln = int(lengths[n])
        for got, want, yard in ((d_points[n, :ln], g64[2 * n], g32[2 * n]), (d_verts[voff[n]:voff[n + 1]], g64[2 * n + 1], g32[2 * n + 1])):
            e_k = float((got.double() - want).abs().max())
            e_y = max(float((yard.double() - want).abs().max()), U * float(want.abs().max()))
            assert e_k <= 4 * e_y, (kind, n, e_k, e_y)
            worst = max(worst, e_k / e_y) if e_y > 0 else worst
        # exactly 0: beyond the cloud's length, without a face, on the surface, on the side the loss ignores - and for the vertices
        # of no other record.  (Not "wherever the reference is 0": on a face whose normal has a zero component autograd returns a
        # structural 0 where the kernel's float64 residual p - c is 1e-17.)
        side = inside[n, :ln]
        dead = (face[n, :ln] < 0) | (dist2[n, :ln] == 0)
        if kind != "sdist":
            ignored = ~side if kind == "penetration" else side
            assert ignored.any() and (~ignored).any()
            dead = dead | ignored
        assert (d_points[n, ln:] == 0).all() and (d_points[n, :ln][dead] == 0).all() and (g64[2 * n][dead] == 0).all(), (kind, n)
        assert (d_points[n, :ln][~dead] != 0).any(-1).all(), (kind, n)
        touched = torch.zeros(len(ms[n][0]), dtype=torch.bool, device=DEV)
        touched[torch.from_numpy(np.asarray(ms[n][1])).to(DEV)[face[n, :ln][~dead]].reshape(-1)] = True
        assert (d_verts[voff[n]:voff[n + 1]][~touched] == 0).all() and (g64[2 * n + 1][~touched] == 0).all(), (kind, n)
    assert (d_points[0, [9, 11]] == 0).all() and (d_points != 0).any() and (d_verts != 0).any()
    _report(f"gradient {kind}", worst_error_over_yardstick=worst)


def test_loss_weights():
    """``weights``: the weighted mean per cloud; zero weights switch points off."""
    from smilify_amd import fit3d

    ms, points, lengths = _gradient_batch()
    meshes, pts, lens = _meshes(*ms), _dev(points), torch.as_tensor(lengths).to(DEV)
    w = torch.from_numpy(np.random.default_rng(98).uniform(0.5, 2.0, (2, 257)).astype(np.float32)).to(DEV)
    d2, face = fit3d.point_face_distance(meshes, pts, lens)
    from smilify_amd import mesh3d

    inside = mesh3d.contains(meshes, pts, lens)
    valid = torch.arange(257, device=DEV)[None] < lens[:, None]
    for fn, counted in ((fit3d.containment_loss, ~inside), (fit3d.penetration_loss, inside)):
        term = torch.where(counted & (face >= 0), d2, torch.zeros_like(d2)).double()
        want = ((term * valid).sum(1) / lens).mean()
        assert abs(float(fn(meshes, pts, lens)) - float(want)) <= 1e-6 * float(want)
        want = ((w.double() * term * valid).sum(1) / (w.double() * valid).sum(1)).mean()
        assert abs(float(fn(meshes, pts, lens, weights=w)) - float(want)) <= 1e-6 * float(want)
    assert float(fit3d.containment_loss(meshes, pts, lens)) > 0 and float(fit3d.penetration_loss(meshes, pts, lens)) > 0


# ---- the optimiser and the Stage ---------------------------------------------------------------------------------------------------------
def test_adam_pulls_a_cloud_into_the_icosphere():
    from smilify_amd import fit3d, mesh3d

    meshes = _meshes(WC.icosphere())
    start = PC.random_cloud(99, 500, 0.45) + np.asarray([0.8, 0.0, 0.0], np.float32)
    pts = _dev(start)[None].requires_grad_(True)
    outside = ~mesh3d.contains(meshes, pts.detach())
    assert 0.3 < float(outside.double().mean()) < 0.7  # it starts half outside
    opt = torch.optim.Adam([pts], lr=0.03)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        loss = fit3d.containment_loss(meshes, pts)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    _report("containment by Adam", start=float(losses[0]), lowest=float(losses.min()), last=float(losses[-1]))
    assert float(losses.min()) < 1e-3 * float(losses[0])
    assert torch.equal(pts.detach()[0][~outside[0]], _dev(start)[~outside[0]])  # the points that were inside never moved


def test_stage_contain_term_and_default_path():
    from smilify_amd import engine, fit3d
    from smilify_amd import visual_hull as VH
    from smilify_amd.mesh3d import Meshes

    def problem():
        torch.manual_seed(0)
        model = fit3d.SMAL3DFitter(batch_size=1, device=DEV, model_path=MODEL_FILES["stick"])
        with torch.no_grad():
            tv = model()
        return model, tv

    # a sphere's hull mesh around the model, off its centre by a third of the model's radius: part of the model starts outside
    model, tv = problem()
    centre = tv[0].mean(0)
    radius = float((tv[0] - centre).norm(dim=-1).max())
    G = WC.HULL_G
    voxel = 0.9 * radius / 4.6  # (a ball smaller than the model's reach: its far end cannot start inside)
    origin = (centre + torch.tensor([0.35, -0.2, 0.1], device=DEV) * radius).double().cpu().numpy() - 0.5 * G * voxel
    occ = torch.from_numpy(WC.hull_occupancy()).to(DEV)
    mesh = VH.VisualHull(occ, None, None, engine.HullGridSpec(1, (G, G, G), tuple(float(x) for x in origin), float(voxel))).extract_mesh(
        relax_steps=VH.taubin_steps(4), return_normals=False)
    target = Meshes([mesh.verts.float()], [mesh.faces.long()])
    stage = fit3d.Stage(30, "init", model, target, lr=0.01 * radius,
                        loss_weights=dict(w_chamfer=0, w_edge=0, w_normal=0, w_laplacian=0, w_contain=1))
    stage.run()
    s = torch.stack(stage.loss_components_to_plot["contain"]).cpu()
    _report("stage contain", first=float(s[0]), last=float(s[-1]))
    assert list(stage.loss_components_to_plot) == ["contain"] and torch.isfinite(s).all() and float(s[0]) > 0 and float(s[-1]) < float(s[0])
    # without the key: the losses of the iteration are those of the terms evaluated here, bit for bit, on the same seed
    model, tv = problem()
    target = Meshes([tv[0] + torch.tensor([0.05, -0.03, 0.02], device=DEV)], [model.faces[0]])
    stage = fit3d.Stage(1, "init", model, target, lr=0.005)
    assert "w_contain" not in stage.loss_weights
    torch.manual_seed(7)
    loss, comps = stage.forward(stage.src_mesh)
    torch.manual_seed(7)
    samples = fit3d.sample_points_from_meshes(target, 3000)
    chamfer, _ = fit3d.chamfer_distance(samples, stage.src_mesh.verts_padded())
    reg = fit3d.mesh_regularisers(stage.src_mesh, True, True, True)
    w = fit3d.default_weights
    want = 0 + w["w_chamfer"] * chamfer
    for name, r in zip(("edge", "normal", "laplacian"), reg.unbind(0)):
        want = want + w[f"w_{name}"] * r
    assert sorted(comps) == ["chamfer", "edge", "laplacian", "normal"] and torch.equal(loss, want)
