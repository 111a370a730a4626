"""GPU tests of the hull's mesh extraction (``pytest -m gpu``): ``VisualHull.extract_mesh`` against the numpy float64 restatement
(tests/hull_mesh_ref.py) on the patterns of tests/distance_field_cases.py.

Conditions.  ``vert_offsets``, ``face_offsets`` and ``faces`` equal the restatement's as integers; two calls give the same bits for every
output.  Shapes: Gx in {1, 2, 62, 63, 64, 127, 130} (Gx + 1 cubes a row: below, on and above one and two waves) x Gy, Gz in {1, 3, 5},
(3, 65, 2) and (2, 3, 130); every pattern (a voxel in each of the 8 corners, two opposite corners, a plane, a checkerboard - every cube
active, every mesh edge 4-fold -, random at 0.5 and 0.01, a full frame, an empty frame between two full ones); origin and voxel size as
the dyadic pair and as a per-frame table of 17 rows; schedules ``()``, ``(0.5,)``, ``gibson_steps(3)``, ``taubin_steps(2)`` and a weight of 0.
One call beyond 2^31 cubes (and voxels).

Values.  The kernel performs the restatement's float64 operations in the restatement's order (no contraction), and division and sqrt
are correctly rounded on both sides, so one rounding to float32 is the whole expected difference: the bound is ``MESH_ULPS`` = 1 float32
ulp of the reference value, for ``verts`` and ``normals`` alike.  Measured on an MI355X over every case below: 0 ulp for both (each test
prints its maximum; DESIGN.md 4.19 records the figure).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import distance_field_cases as DC
import hull_mesh_ref as MR
import visual_hull_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MESH_ULPS = 1.0  # (the project's SAMPLER_ULPS construction, tests/test_gpu_distance_field.py)
DYADIC = ((-1.5, 0.25, -0.75), 0.125)
SCHEDULES = [(), (0.5,), MR.gibson_steps(3), MR.taubin_steps(2), (0.0,)]
GX = (1, 2, 62, 63, 64, 127, 130)
SHAPES = [(gx, gy, gz) for gx in GX for gy in (1, 3, 5) for gz in (1, 3, 5)] + [(3, 65, 2), (2, 3, 130)]


def _per_frame(N, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (N, 3)), rng.uniform(0.04, 0.13, N)


def _hull(occ, origin=(0.0, 0.0, 0.0), voxel=1.0):
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH

    occ = occ if isinstance(occ, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(occ)).to(DEV)
    N, Gz, Gy, Gx = occ.shape
    return VH.VisualHull(occ, None, None, engine.HullGridSpec(N, (Gx, Gy, Gz), origin, voxel))


@functools.lru_cache(maxsize=4)
def _tops(G):
    return MR.topologies(DC.patterns(G))


def _ulps(got, ref64):
    ref = ref64.astype(np.float32)
    if not ref.size:
        return 0.0
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())


def _fields(mesh):
    return [t for t in (mesh.verts, mesh.normals, mesh.faces, mesh.vert_offsets, mesh.face_offsets) if t is not None]


def _check(mesh, ref, what):
    """Integers equal, values within MESH_ULPS; returns the two measured maxima."""
    assert mesh.verts.dtype == mesh.normals.dtype == torch.float32 and mesh.faces.dtype == mesh.vert_offsets.dtype == mesh.face_offsets.dtype == torch.int64
    assert np.array_equal(mesh.vert_offsets.cpu().numpy(), ref.vert_offsets), what
    assert np.array_equal(mesh.face_offsets.cpu().numpy(), ref.face_offsets), what
    assert tuple(mesh.verts.shape) == ref.verts.shape == tuple(mesh.normals.shape) and tuple(mesh.faces.shape) == ref.faces.shape, what
    bad = mesh.faces.cpu().numpy() != ref.faces
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return _ulps(mesh.verts.cpu().numpy(), ref.verts), _ulps(mesh.normals.cpu().numpy(), ref.normals)


@pytest.mark.parametrize("Gx", sorted({G[0] for G in SHAPES}))
def test_grid_shapes(Gx):
    """Every pattern (17 frames a call) x tables x schedule on the grids with this Gx.  Measured on an MI355X: 0 ulp for vertices and
    normals alike, over every shape."""
    worst = [0.0, 0.0]
    for G in (g for g in SHAPES if g[0] == Gx):
        occ = DC.patterns(G)
        tops = _tops(G)
        dev_occ = torch.from_numpy(occ).to(DEV)
        for weights in SCHEDULES:
            positions = [MR.relax(top, weights) for top in tops]
            for origin, voxel in (DYADIC, _per_frame(len(occ))):
                hull = _hull(dev_occ, origin, voxel)
                mesh = hull.extract_mesh(weights)
                ref = MR.assemble(tops, positions, origin, voxel)
                v, n = _check(mesh, ref, (G, weights))
                worst = [max(worst[0], v), max(worst[1], n)]
        again = hull.extract_mesh(weights)  # two calls: the same bits
        assert all(torch.equal(a, b) for a, b in zip(_fields(mesh), _fields(again))), G
        e = DC.NAMES.index("empty")
        assert int(mesh.vert_offsets[e]) == int(mesh.vert_offsets[e + 1]) and int(mesh.face_offsets[e]) == int(mesh.face_offsets[e + 1])
    print(f"Gx = {Gx}: max error {worst[0]:.3g} ulp (vertices), {worst[1]:.3g} ulp (normals)")
    assert max(worst) <= MESH_ULPS


def test_without_normals_and_an_empty_hull():
    G = (7, 5, 3)
    occ = DC.patterns(G)
    hull = _hull(occ, *DYADIC)
    full = hull.extract_mesh(MR.taubin_steps(2))
    plain = hull.extract_mesh(MR.taubin_steps(2), return_normals=False)
    assert plain.normals is None and torch.equal(plain.verts, full.verts) and torch.equal(plain.faces, full.faces)
    with pytest.raises(ValueError, match="return_normals=False"):
        plain.normals_list()
    # the lists, the volume and the meshes
    ref = MR.extract(occ, *DYADIC, MR.taubin_steps(2), tops=_tops(G))
    vl, fl, nl = full.verts_list(), full.faces_list(), full.normals_list()
    assert len(vl) == len(fl) == len(nl) == len(full) == len(occ)
    volume = full.volume()
    assert volume.dtype == torch.float64 and tuple(volume.shape) == (len(occ),)
    for n in range(len(occ)):
        v, f = slice(ref.vert_offsets[n], ref.vert_offsets[n + 1]), slice(ref.face_offsets[n], ref.face_offsets[n + 1])
        assert tuple(vl[n].shape) == (v.stop - v.start, 3) and torch.equal(fl[n], full.faces[f]) and torch.equal(nl[n], full.normals[v])
        want = MR.signed_volume(vl[n].cpu().numpy().astype(np.float64), ref.faces[f]) if f.stop > f.start else 0.0
        assert abs(float(volume[n]) - want) <= 1e-12 * max(abs(want), 1e-3), (n, float(volume[n]), want)
        assert (want > 0.0) == bool(occ[n].any())
    empty = [n for n in range(len(occ)) if not occ[n].any()]  # (at 0.01 the random frame of this grid is empty too)
    assert DC.NAMES.index("empty") in empty
    with pytest.raises(ValueError, match=f"frame {empty[0]} has an empty hull"):
        full.to_meshes()
    keep = [n for n in range(len(occ)) if n not in empty]
    meshes = full.to_meshes(keep=keep)
    assert len(meshes) == len(keep) and meshes.num_verts_per_mesh() == [int(vl[n].shape[0]) for n in keep]
    assert meshes.num_faces_per_mesh() == [int(fl[n].shape[0]) for n in keep]
    # an all-empty hull: zero totals, nothing written
    nothing = _hull(np.zeros((3, 4, 5, 6), np.uint8), *DYADIC).extract_mesh(MR.gibson_steps(2))
    assert tuple(nothing.verts.shape) == tuple(nothing.normals.shape) == (0, 3) and tuple(nothing.faces.shape) == (0, 3)
    assert nothing.vert_offsets.tolist() == [0] * 4 and nothing.face_offsets.tolist() == [0] * 4
    assert nothing.volume().tolist() == [0.0] * 3 and nothing.verts_list()[1].shape[0] == 0


def test_offsets_across_scan_rounds():
    """The scan of the per-workgroup vertex and quad counts takes 1 024 counts a round (a workgroup counts 2 048 cubes).  11 frames of
    63 x 63 x 51 voxels = 64 x 64 x 52 cubes: 104 counts a frame, 1 144 in all - frame 10 starts at count 1 040, inside the second round,
    whose prefixes carry the first round's totals.  Occupancy built directly (``scan_occupancy``: frame 2 empty)."""
    N, G = 11, (63, 63, 51)
    blocks = -(-(G[0] + 1) * (G[1] + 1) * (G[2] + 1) // 2048)
    assert N * blocks == 1144 and 10 * blocks == 1040
    occ = VC.scan_occupancy(N, G)
    hull = _hull(occ, *DYADIC)
    tops = MR.topologies(occ)
    for weights in ((), (0.5,)):
        ref = MR.extract(occ, *DYADIC, weights, tops=tops)
        assert ref.vert_offsets[2] == ref.vert_offsets[3] and (np.diff(ref.vert_offsets)[[0, 1, *range(3, N)]] > 100).all()
        v, n = _check(hull.extract_mesh(weights), ref, weights)
        print(f"weights {weights}: max error {v:.3g} ulp (vertices), {n:.3g} ulp (normals)")
        assert max(v, n) <= MESH_ULPS


def test_beyond_2_31_cubes():
    """N = 33 600 frames of 40^3 voxels = 41^3 cubes (2.15e9 voxels, 2.32e9 cubes; 2.2 GB of occupancy): all empty but the first, the
    last and the two around cube 2^31 and around voxel 2^31, which hold a seeded blob each and are compared with the restatement."""
    N, G = 33_600, 40
    vox, cubes = G ** 3, (G + 1) ** 3
    assert N * vox > 2**31 and N * cubes > 2**31
    by_cube, by_voxel = 2**31 // cubes, 2**31 // vox
    frames = [0, by_cube - 1, by_cube, by_voxel - 1, by_voxel, N - 1]
    assert sorted(set(frames)) == frames
    rng = np.random.default_rng(2031)
    small = np.stack([DC.blob((G, G, G), 1, seed=s)[0] for s in range(len(frames))])
    small |= (rng.random(small.shape) < 0.002).astype(np.uint8)
    occ = torch.zeros(N, G, G, G, dtype=torch.uint8, device=DEV)
    occ[frames] = torch.from_numpy(small).to(DEV)
    weights = MR.taubin_steps(1)
    mesh = _hull(occ, *DYADIC).extract_mesh(weights)
    ref = MR.extract(small, *DYADIC, weights)
    vo, fo = mesh.vert_offsets.cpu().numpy(), mesh.face_offsets.cpu().numpy()
    assert all(r > 1000 for r in np.diff(ref.vert_offsets))
    sizes = np.zeros(N, np.int64)
    sizes[frames] = np.diff(ref.vert_offsets)
    assert np.array_equal(np.diff(vo), sizes) and vo[0] == 0
    sizes[frames] = np.diff(ref.face_offsets)
    assert np.array_equal(np.diff(fo), sizes) and fo[0] == 0
    assert np.array_equal(mesh.faces.cpu().numpy(), ref.faces)
    assert _ulps(mesh.verts.cpu().numpy(), ref.verts) <= MESH_ULPS and _ulps(mesh.normals.cpu().numpy(), ref.normals) <= MESH_ULPS


def test_argument_errors():
    from smilify_amd import _lib, engine

    occ = torch.from_numpy(DC.patterns((4, 3, 2))).to(DEV)
    N = occ.shape[0]
    spec = engine.HullGridSpec(N, (4, 3, 2), *DYADIC)
    for value in (float("nan"), float("inf")):
        with pytest.raises(_lib.SmilError, match=r"weights\[1\].*finite"):
            engine.hull_mesh(spec, occ, (0.5, value))
    with pytest.raises(_lib.SmilError, match="positive and finite"):
        engine.hull_mesh(engine.HullGridSpec(N, (4, 3, 2), DYADIC[0], 0.0), occ)
    with pytest.raises(_lib.SmilError, match="must be finite"):
        engine.hull_mesh(engine.HullGridSpec(N, (4, 3, 2), (0.0, float("nan"), 0.0), 0.1), occ)
    with pytest.raises(_lib.SmilError, match="origin has 2 rows"):
        engine.hull_mesh(engine.HullGridSpec(N, (4, 3, 2), np.zeros((2, 3)), 0.1), occ)
    with pytest.raises(_lib.SmilError, match="voxel_size has 2 rows"):
        engine.hull_mesh(engine.HullGridSpec(N, (4, 3, 2), DYADIC[0], (0.1, 0.1)), occ)
    with pytest.raises(ValueError, match="occ must be a uint8"):
        engine.hull_mesh(spec, occ[:, :1])
    with pytest.raises(ValueError, match="occ must be a uint8"):
        engine.hull_mesh(spec, occ.to(torch.int32))
    # the calls themselves, on real buffers
    lib = _lib.load()
    grid = ctypes.byref(spec.struct)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ws = torch.empty(int(lib.smil_hull_mesh_workspace_bytes(grid)), dtype=torch.uint8, device=DEV)
    off = torch.empty(2, N + 1, dtype=torch.int64, device=DEV)
    for args in ((None, ptr(off[0]), ptr(off[1]), ptr(ws)), (ptr(occ), None, ptr(off[1]), ptr(ws)), (ptr(occ), ptr(off[0]), None, ptr(ws)),
                 (ptr(occ), ptr(off[0]), ptr(off[1]), None)):
        with pytest.raises(_lib.SmilError, match="null argument"):
            _lib.check(lib.smil_hull_mesh_count(grid, *args, None), "smil_hull_mesh_count")
    with pytest.raises(_lib.SmilError, match="null grid"):
        _lib.check(lib.smil_hull_mesh_count(None, ptr(occ), ptr(off[0]), ptr(off[1]), ptr(ws), None), "smil_hull_mesh_count")
    huge = engine.HullGridSpec(1, (2047, 1023, 1023), *DYADIC)  # 2^31 cubes: refused before anything is read
    with pytest.raises(_lib.SmilError, match=r"2\^31 or more cubes"):
        _lib.check(lib.smil_hull_mesh_count(ctypes.byref(huge.struct), ptr(occ), ptr(off[0]), ptr(off[1]), ptr(ws), None), "smil_hull_mesh_count")
    assert lib.smil_hull_mesh_workspace_bytes(ctypes.byref(huge.struct)) == 0
    _lib.check(lib.smil_hull_mesh_count(grid, ptr(occ), ptr(off[0]), ptr(off[1]), ptr(ws), None), "smil_hull_mesh_count")
    nv, nf = (int(t) for t in off[:, -1].tolist())
    assert nv > 0 and nf > 0
    scratch = torch.empty(int(lib.smil_hull_mesh_scratch_bytes(nv, 2)), dtype=torch.uint8, device=DEV)
    verts = torch.full((nv, 3), 7.0, dtype=torch.float32, device=DEV)
    faces = torch.full((nf, 3), -7, dtype=torch.int64, device=DEV)
    w = np.array([0.5, -0.53])

    def write(**over):
        a = dict(occ=ptr(occ), ws=ptr(ws), scratch=ptr(scratch), nv=nv, nf=nf, weights=w.ctypes.data, steps=2, verts=ptr(verts), faces=ptr(faces))
        a.update(over)
        return lib.smil_hull_mesh_write(grid, a["occ"], a["ws"], a["scratch"], a["nv"], a["nf"], a["weights"], a["steps"], a["verts"], None, a["faces"],
                                        None)

    for over, text in ((dict(steps=-1), "n_steps=-1"), (dict(weights=None), "null weights"), (dict(nv=-1), "not counts of this grid"),
                       (dict(nf=-1), "not counts of this grid"), (dict(occ=None), "null occ or workspace"), (dict(ws=None), "null occ or workspace"),
                       (dict(scratch=None), "null scratch, verts or faces"), (dict(verts=None), "null scratch, verts or faces"),
                       (dict(faces=None), "null scratch, verts or faces")):
        with pytest.raises(_lib.SmilError, match=text):
            _lib.check(write(**over), "smil_hull_mesh_write")
    # figures that are not the workspace's own: accepted, and nothing is written
    _lib.check(write(nv=nv - 1), "smil_hull_mesh_write")
    _lib.check(write(nf=nf - 2), "smil_hull_mesh_write")
    torch.cuda.synchronize()
    assert bool((verts == 7.0).all()) and bool((faces == -7).all())
    _lib.check(write(), "smil_hull_mesh_write")
    ref = MR.extract(DC.patterns((4, 3, 2)), *DYADIC, tuple(w))
    assert np.array_equal(faces.cpu().numpy(), ref.faces) and _ulps(verts.cpu().numpy(), ref.verts) <= MESH_ULPS


def test_carved_sphere_feeds_the_mesh_side():
    """A sphere carved from 6 synthetic views at 32^3, meshed with ``taubin_steps(5)``: the sampler returns finite points and unit normals,
    the ray-cast diameters are finite, positive and below the grid's diagonal, and the chamfer distance between mesh samples and the
    hull's surface voxels is below one voxel squared."""
    from smilify_amd import fit3d, sdf
    from smilify_amd import visual_hull as VH

    voxel, radius = 0.05, 0.45
    c = VC._case("mesh_sphere", views=6, grid=(32, 32, 32), voxel=voxel, origin=(-0.8137, -0.7911, -0.8023), min_views=6, fov=27.0, elev=(-20.0, 30.0),
                 ellipsoids=((VC.ELLIPSOID[0], np.full(3, radius)),), seed=77)
    hull = VH.carve(torch.from_numpy(c.masks).to(DEV), {k: torch.from_numpy(v) for k, v in c.cams.items()}, image_size=c.S, origin=c.origin,
                    voxel_size=c.voxel_size, grid=c.grid, min_views=c.min_views)
    assert int(hull.occupancy.sum()) > 2000
    mesh = hull.extract_mesh(VH.taubin_steps(5))
    volume = float(mesh.volume()[0])
    ball = 4.0 / 3.0 * np.pi * radius ** 3
    print(f"sphere: {mesh.verts.shape[0]} vertices, {mesh.faces.shape[0]} faces, volume {volume:.4f} (the ball's {ball:.4f})")
    assert 0.9 * ball < volume < 1.6 * ball  # a visual hull contains its object; six views leave it some corners
    centre = torch.from_numpy(VC.ELLIPSOID[0]).to(DEV, torch.float32)
    assert bool(((mesh.normals * (mesh.verts - centre)).sum(1) > 0).all())
    meshes = mesh.to_meshes()
    S = 10_000
    points, normals = fit3d.sample_points_from_meshes(meshes, S, return_normals=True)
    assert tuple(points.shape) == tuple(normals.shape) == (1, S, 3) and bool(torch.isfinite(points).all())
    assert bool(((normals.norm(dim=-1) - 1.0).abs() < 1e-5).all())
    assert bool(((normals * (points - centre)).sum(-1) > 0).float().mean() > 0.99)
    torch.manual_seed(3)
    where, diameters = sdf.compute_sdf(meshes, num_samples=500, num_rays=10)
    diagonal = voxel * 32 * np.sqrt(3.0)
    assert tuple(diameters.shape) == (500,) and bool(torch.isfinite(diameters).all()) and bool((diameters > 0).all())
    assert float(diameters.max()) < diagonal
    loss, _ = fit3d.chamfer_distance(points, hull.sample_surface(S, seed=1))
    print(f"sphere: chamfer {float(loss):.6f} against one voxel squared {voxel * voxel:.6f}")
    assert float(loss) < voxel * voxel
