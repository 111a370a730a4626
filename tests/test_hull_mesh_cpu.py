"""CPU checks of the hull's mesh extraction (no GPU): the numpy restatement (tests/hull_mesh_ref.py) against first principles, and the
argument validation of the C ABI through ctypes.

First principles.  A single voxel gives 8 vertices and 12 triangles: the cube of a third of the voxel's edge (unrelaxed surface nets cut
every corner).  A full ``Gx x Gy x Gz`` grid gives ``2 (Gx Gy + Gy Gz + Gx Gz)`` quads.  On every pattern of
``distance_field_cases.patterns``: each directed edge a->b occurs as often as b->a (closed and consistently oriented - a checkerboard's
4-fold edges included), the signed volume is positive, every emitted vertex is used, every vertex lies in its own cube after any
schedule, and frames do not leak into each other.  On a voxel ball (radius 4.6 in 12^3, 432 voxels) relaxation lowers the spread of
the vertex radii and Taubin's schedule keeps the volume (measured: std 0.133 / 0.071 / 0.089 and volume 412 / 376 / 418 for no
relaxation / ``gibson_steps(4)`` / ``taubin_steps(10)``).
"""
import ctypes
from collections import Counter

import numpy as np
import pytest

import distance_field_cases as DC
import hull_mesh_ref as MR

WILD = (7.5, -3.0)
SCHEDULES = [(), (0.5,), MR.gibson_steps(3), MR.taubin_steps(2), (0.0,), WILD]
SHAPES = [(1, 1, 1), (2, 1, 3), (4, 4, 4), (7, 5, 3), (3, 65, 2)]


def _frames(m):
    for n in range(len(m.vert_offsets) - 1):
        v = slice(m.vert_offsets[n], m.vert_offsets[n + 1])
        yield n, m.verts[v], m.index[v], m.cubes[v], m.faces[m.face_offsets[n]:m.face_offsets[n + 1]]


def _closed_and_oriented(faces):
    edges = Counter(map(tuple, np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).tolist()))
    return all(edges[(b, a)] == k for (a, b), k in edges.items()), max(edges.values(), default=0)


def test_single_voxel_is_a_third_of_a_cube():
    from smilify_amd import visual_hull as VH

    assert VH.gibson_steps(3) == MR.gibson_steps(3) == (0.5, 0.5, 0.5) and VH.taubin_steps(2) == MR.taubin_steps(2) == (0.5, -0.53, 0.5, -0.53)
    occ = np.zeros((1, 3, 3, 3), np.uint8)
    occ[0, 1, 1, 1] = 1
    voxel = 0.5
    m = MR.extract(occ, (0.0, 0.0, 0.0), voxel)
    assert len(m.verts) == 8 and len(m.faces) == 12
    centre = 1.5 * voxel
    assert np.allclose(np.abs(m.verts - centre), voxel / 6.0, rtol=0, atol=1e-15)  # corners of a cube of edge voxel / 3
    assert abs(MR.signed_volume(m.verts, m.faces) - voxel ** 3 / 27.0) < 1e-15
    assert np.allclose(m.normals, (m.verts - centre) / np.linalg.norm(m.verts - centre, axis=1, keepdims=True), atol=1e-15)
    assert _closed_and_oriented(m.faces) == (True, 1)
    alone = MR.extract(np.ones((1, 1, 1, 1), np.uint8), (0.0, 0.0, 0.0), voxel)  # the grid's border is outside: the same cube
    assert np.array_equal(alone.faces, m.faces) and np.allclose(alone.verts + voxel, m.verts, rtol=0, atol=1e-15)


@pytest.mark.parametrize("G", [(1, 1, 1), (2, 2, 2), (5, 3, 2), (9, 1, 4), (6, 7, 4)])
def test_full_grid_counts(G):
    Gx, Gy, Gz = G
    occ = np.ones((1, Gz, Gy, Gx), np.uint8)
    m = MR.extract(occ)
    quads = 2 * (Gx * Gy + Gy * Gz + Gx * Gz)
    assert len(m.faces) == 2 * quads == 4 * (Gx * Gy + Gy * Gz + Gx * Gz)
    assert len(m.verts) == (Gx + 1) * (Gy + 1) * (Gz + 1) - max(Gx - 1, 0) * max(Gy - 1, 0) * max(Gz - 1, 0)
    # The box of the voxels, minus what the unrelaxed vertices cut off it: a vertex on one of the box's 12 edges sits a quarter of a
    # voxel inside both faces - between the vertices of two neighbouring voxels that costs 4 x 1/4 = 1 per axis and voxel step - and the
    # 8 corner pieces cost 9/8 together (every extent >= 2; an axis of one voxel rounds the whole slab, see the single voxel).
    volume = MR.signed_volume(m.verts, m.faces)
    box = float(Gx * Gy * Gz)
    assert _closed_and_oriented(m.faces)[0] and 0.0 < volume < box
    print(f"full {G}: volume {volume:.6f} of box {box:.0f}, {len(m.verts)} vertices, {quads} quads")
    if min(G) >= 2:
        assert abs(volume - (box - ((Gx - 1) + (Gy - 1) + (Gz - 1)) - 9.0 / 8.0)) <= 1e-12 * box


@pytest.mark.parametrize("G", SHAPES, ids=lambda G: "x".join(map(str, G)))
def test_patterns_closed_oriented_used_and_clamped(G):
    occ = DC.patterns(G)
    tops = MR.topologies(occ)
    names = DC.NAMES
    for weights in SCHEDULES:
        m = MR.extract(occ, (-1.5, 0.25, -0.75), 0.125, weights, tops=tops)
        for n, verts, index, cubes, faces in _frames(m):
            empty = not occ[n].any()
            assert (len(verts) == 0) == empty and (len(faces) == 0) == empty, (G, names[n])
            if empty:
                continue
            ok, fold = _closed_and_oriented(faces)
            assert ok, (G, names[n], weights)
            assert fold in (1, 2), (G, names[n], fold)  # 2: an edge shared by four quads, where voxels touch along an edge only
            if weights != WILD:  # (weights beyond 1 only test the clamp: they may fold the mesh flat)
                assert MR.signed_volume(verts, faces) > 0.0, (G, names[n], weights)
            assert np.array_equal(np.unique(faces), np.arange(len(verts))), (G, names[n])
            assert (index >= cubes).all() and (index <= cubes + 1).all(), (G, names[n], weights)
            length = np.linalg.norm(m.normals[m.vert_offsets[n]:m.vert_offsets[n + 1]], axis=1)
            assert ((np.abs(length - 1.0) < 1e-12) | (length == 0.0)).all()
    # frames do not leak: the empty frame between two full ones, and the two full ones alike
    m = MR.extract(occ, weights=MR.gibson_steps(2), tops=tops)
    e = names.index("empty")
    assert m.vert_offsets[e] == m.vert_offsets[e + 1] and m.face_offsets[e] == m.face_offsets[e + 1]
    a, b = names.index("full_a"), names.index("full_b")
    assert np.array_equal(m.verts[m.vert_offsets[a]:m.vert_offsets[a + 1]], m.verts[m.vert_offsets[b]:m.vert_offsets[b + 1]])
    assert np.array_equal(m.faces[m.face_offsets[a]:m.face_offsets[a + 1]], m.faces[m.face_offsets[b]:m.face_offsets[b + 1]])
    alone = MR.extract(occ[a:a + 1], weights=MR.gibson_steps(2))
    assert np.array_equal(alone.verts, m.verts[m.vert_offsets[a]:m.vert_offsets[a + 1]]) and np.array_equal(alone.faces, m.faces[m.face_offsets[a]:m.face_offsets[a + 1]])


def test_checkerboard_is_the_worst_case():
    """Every cube is active but the 4 corner cubes whose one grid sample is empty, and mesh edges are 4-fold."""
    G = (4, 4, 4)
    occ = DC.patterns(G)[DC.NAMES.index("checker")][None]
    m = MR.extract(occ)
    assert len(m.verts) == 5 ** 3 - 4
    ok, fold = _closed_and_oriented(m.faces)
    assert ok and fold == 2


def test_ball_relaxation_smooths_and_taubin_keeps_the_volume():
    occ = MR.ball(12, 4.6)
    voxels = int(occ.sum())
    assert voxels == 432
    top = MR.topologies(occ)
    centre = 6.0  # the grid's centre in world units (origin 0, voxel 1)
    out = {}
    for name, weights in (("unrelaxed", ()), ("gibson", MR.gibson_steps(4)), ("taubin", MR.taubin_steps(10))):
        m = MR.extract(occ, weights=weights, tops=top)
        radius = np.linalg.norm(m.verts - centre, axis=1)
        out[name] = (float(radius.std()), MR.signed_volume(m.verts, m.faces))
        length = np.linalg.norm(m.normals, axis=1)
        assert (np.abs(length - 1.0) < 1e-12).all()
        assert ((m.normals * (m.verts - centre)).sum(1) > 0.0).all(), name
        print(f"ball {name}: radius std {out[name][0]:.4f}, volume {out[name][1]:.2f} ({voxels} voxels)")
    assert out["gibson"][0] < out["unrelaxed"][0] and out["taubin"][0] < out["unrelaxed"][0]
    slack = abs(out["unrelaxed"][1] - voxels)
    assert abs(out["taubin"][1] - out["unrelaxed"][1]) <= slack


def test_midpoints_are_what_the_distance_field_would_interpolate():
    """Across a sign-changing lattice edge both squared distances are 1, so a crossing interpolated from the signed field
    sqrt(d2_out) - sqrt(d2_in) lies at the midpoint: occupancy is all the extraction needs."""
    import distance_field_ref as DR

    occ = DC.patterns((5, 4, 3))
    d_out, d_in = DR.edt_brute(occ, 0, 0), DR.edt_brute(occ, 1, 1)
    inside = occ != 0
    for axis in (1, 2, 3):
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        change = inside[lo] != inside[hi]
        field = np.sqrt(np.where(d_out == DR.NONE, 0, d_out).astype(np.float64)) - np.sqrt(d_in.astype(np.float64))
        f0, f1 = field[lo][change], field[hi][change]
        assert change.any() and np.array_equal(np.abs(f0), np.ones_like(f0)) and np.array_equal(f0, -f1)
        assert np.array_equal(f0 / (f0 - f1), np.full_like(f0, 0.5))


# ---- the C ABI's argument validation (no GPU: every call fails before its first launch) -------------------------------------------
def _grid(lib_mod, N=1, G=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=(0.1,)):
    o = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(-1, 3))
    s = np.ascontiguousarray(np.asarray(voxel, np.float64).reshape(-1))
    g = lib_mod.HullGrid()
    g.N, (g.Gx, g.Gy, g.Gz) = N, G
    g.origin, g.n_origin, g.voxel_size, g.n_voxel_size = o.ctypes.data, o.shape[0], s.ctypes.data, s.shape[0]
    return g, (o, s)


def test_mesh_argument_validation_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    assert b"hull meshes" in lib.smil_version()
    for name in ("smil_hull_mesh_workspace_bytes", "smil_hull_mesh_count", "smil_hull_mesh_scratch_bytes", "smil_hull_mesh_write"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data  # a non-null stand-in: nothing is dereferenced before the arguments are accepted
    err = lambda: lib.smil_last_error()  # noqa: E731
    w = np.array([0.5, -0.53])

    def count(g, occ=p, vo=p, fo=p, ws=p):
        return lib.smil_hull_mesh_count(ctypes.byref(g), occ, vo, fo, ws, None)

    def write(g, occ=p, ws=p, scratch=p, nv=8, nf=12, weights=w.ctypes.data, steps=2, verts=p, normals=None, faces=p):
        return lib.smil_hull_mesh_write(ctypes.byref(g), occ, ws, scratch, nv, nf, weights, steps, verts, normals, faces, None)

    g, keep = _grid(_lib)
    for G in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        gb, kb = _grid(_lib, G=G)
        assert count(gb) == -1 and b"below 1" in err(), err()
        assert write(gb) == -1 and b"below 1" in err(), err()
        assert lib.smil_hull_mesh_workspace_bytes(ctypes.byref(gb)) == 0
    gb, kb = _grid(_lib, N=0)
    assert count(gb) == -1 and b"N=0" in err(), err()
    gb, kb = _grid(_lib, G=(1 << 20, 1 << 20, 2))
    assert count(gb) == -1 and b"2^40" in err(), err()
    gb, kb = _grid(_lib, G=(2047, 1023, 1023))  # 2^31 cubes
    assert count(gb) == -1 and b"2^31 or more cubes" in err(), err()
    assert write(gb) == -1 and b"2^31 or more cubes" in err(), err()
    gb, kb = _grid(_lib, N=1 << 20, G=(127, 127, 127))  # 2^20 frames of 2^21 cubes: 2^30 workgroups
    assert count(gb) == -1 and b"exceed the grid" in err(), err()
    assert lib.smil_hull_mesh_count(None, p, p, p, p, None) == -1 and b"null grid" in err()
    for bad in (dict(occ=None), dict(vo=None), dict(fo=None), dict(ws=None)):
        assert count(g, **bad) == -1 and b"null argument" in err(), (bad, err())
    # the write reads the tables
    for voxel in (0.0, -0.1, float("nan"), float("inf")):
        gb, kb = _grid(_lib, voxel=(voxel,))
        assert write(gb) == -1 and b"must be positive and finite" in err(), err()
    gb, kb = _grid(_lib, origin=(0.0, float("inf"), 0.0))
    assert write(gb) == -1 and b"must be finite" in err(), err()
    gb, kb = _grid(_lib, N=3, origin=np.zeros((2, 3)))
    assert write(gb) == -1 and b"origin has 2 rows" in err(), err()
    gb, kb = _grid(_lib, N=3, voxel=(0.1, 0.1))
    assert write(gb) == -1 and b"voxel_size has 2 rows" in err(), err()
    assert write(g, steps=-1) == -1 and b"n_steps=-1" in err(), err()
    assert write(g, weights=None) == -1 and b"null weights" in err(), err()
    for value in (float("nan"), float("inf"), -float("inf")):
        bad = np.array([0.5, value])
        assert write(g, weights=bad.ctypes.data) == -1 and b"weights[1]" in err() and b"finite" in err(), err()
    assert write(g, nv=-1) == -1 and b"not counts of this grid" in err(), err()
    assert write(g, nf=-2) == -1 and b"not counts of this grid" in err(), err()
    assert write(g, nv=1 << 40) == -1 and b"not counts of this grid" in err(), err()
    assert write(g, occ=None) == -1 and b"null occ or workspace" in err(), err()
    assert write(g, ws=None) == -1 and b"null occ or workspace" in err(), err()
    for bad in (dict(scratch=None), dict(verts=None), dict(faces=None)):
        assert write(g, **bad) == -1 and b"null scratch, verts or faces" in err(), (bad, err())
    # sizes: 5^3 = 125 cubes are one workgroup of 32 words: 2 x (1 + 1) int64 prefixes, the two tables, 32 masks, 32 word prefixes
    assert lib.smil_hull_mesh_workspace_bytes(ctypes.byref(g)) == 3 * 256 + 256 + 256 and lib.smil_hull_mesh_workspace_bytes(None) == 0
    assert lib.smil_hull_mesh_scratch_bytes(8, 0) == 3 * 256 and lib.smil_hull_mesh_scratch_bytes(8, 3) == 4 * 256
    assert lib.smil_hull_mesh_scratch_bytes(-1, 0) == 0 and lib.smil_hull_mesh_scratch_bytes(8, -1) == 0
    assert lib.smil_hull_mesh_scratch_bytes(0, 0) == 0
    # nothing to write: accepted without a launch (and so without a GPU)
    assert write(g, nv=0, nf=0, scratch=None, verts=None, faces=None) == 0
