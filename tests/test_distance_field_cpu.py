"""CPU checks of the distance fields (no GPU): the numpy restatement (tests/distance_field_ref.py) against scipy's exact transform and
against closed forms, its sampler's gradient against central differences, that the seeded cases hold what the GPU tests lean on, and the
argument validation of the C ABI through ctypes.
"""
import ctypes

import numpy as np
import pytest

import distance_field_cases as DC
import distance_field_ref as DR

CPU_SHAPES = [(1, 1, 1), (2, 1, 1), (5, 3, 1), (7, 6, 5), (65, 3, 2), (2, 3, 33)]


def test_brute_against_scipy():
    """``edt_brute`` = ``scipy.ndimage.distance_transform_edt`` squared and rounded, on every pattern, inverted or not; with ``border`` the
    grid is padded by one voxel of features and the result cropped.  An input without a feature is left out (scipy's result is
    undefined there): ``test_closed_forms`` covers it."""
    ndi = pytest.importorskip("scipy.ndimage")
    for G in CPU_SHAPES:
        occ = DC.patterns(G)
        for invert, border in DC.COMBOS:
            got = DR.edt_brute(occ, invert, border)
            for n in range(len(occ)):
                feat = (occ[n] == 0) if invert else (occ[n] != 0)
                if border:
                    feat = np.pad(feat, 1, constant_values=True)
                if not feat.any():
                    assert (got[n] == DR.NONE).all()
                    continue
                want = np.rint(ndi.distance_transform_edt(~feat) ** 2).astype(np.int64)
                if border:
                    want = want[1:-1, 1:-1, 1:-1]
                assert np.array_equal(got[n], want), (G, invert, border, DC.NAMES[n])


def test_shell_distance_is_the_pairs():
    for G in CPU_SHAPES + [(9, 1, 4)]:
        occ = np.zeros((1, G[2], G[1], G[0]), np.uint8)
        assert np.array_equal(DR.edt_brute(occ, 0, 1)[0], DR.shell_distance(G)), G
    for G in [(7, 6, 5), (65, 3, 2)]:
        for plain, inverted in zip(*DC.sparse_patterns(G, seed=5)):
            for invert, border in DC.COMBOS:
                o = (inverted if invert else plain)[None]
                assert np.array_equal(DR.edt_brute(o, invert, border), DR.edt_brute(o, invert, border, shell_pairs=False))


def test_closed_forms():
    for G in CPU_SHAPES:
        Gx, Gy, Gz = G
        occ = DC.patterns(G)
        k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
        d = DR.edt_brute(occ, 0, 0)
        assert np.array_equal(d[0], i * i + j * j + k * k)  # a single feature at the corner (0, 0, 0)
        assert np.array_equal(d[7], (Gx - 1 - i) ** 2 + (Gy - 1 - j) ** 2 + (Gz - 1 - k) ** 2)
        assert (d[15] == DR.NONE).all() and (d[14] == 0).all() and (d[16] == 0).all()  # the empty frame between two full ones
        inside = DR.edt_brute(occ, 1, 1)
        want = np.minimum(np.minimum(np.minimum(i + 1, Gx - i), np.minimum(j + 1, Gy - j)), np.minimum(k + 1, Gz - k)) ** 2
        assert np.array_equal(inside[13], want)  # a full grid, inverted, with the border
        assert (DR.edt_brute(occ, 1, 0)[13] == DR.NONE).all()
        assert d.dtype == np.int64 and d.max() <= DR.NONE


def test_cases_hold_what_they_are_for():
    assert len(DC.SHAPES) == 56 and (3, 65, 2) in DC.SHAPES and (2, 3, 130) in DC.SHAPES
    occ = DC.patterns((65, 5, 3))
    assert occ.shape[0] == len(DC.NAMES) == 17 and occ[15].sum() == 0 and occ[14].all() and occ[16].all()
    assert 0.4 < (occ[11] != 0).mean() < 0.6 and 0 < (occ[12] != 0).mean() < 0.03 and occ[11].max() == 255
    planes = {G: G[0] * G[1] for G in DC.PATH_SHAPES}
    assert sorted(planes.values())[0] <= 4096 < planes[(130, 33, 2)] <= 16384 < planes[(129, 128, 1)] <= DC.LDS_SLICE
    assert planes[(257, 256, 2)] > DC.LDS_SLICE and planes[(128, DC.LDS_LINE + 1, 1)] > DC.LDS_SLICE
    for G in DC.PATH_SHAPES:
        plain, inverted = DC.sparse_patterns(G)
        assert plain[1].sum() == 0 and inverted[1].all() and plain[0].any() and plain[2].any() and np.array_equal(plain == 0, inverted != 0)
    pts = DC.sample_points((5, 3, 4), (-1.5, 0.25, -0.75), 0.125, 2, 65, 3)
    u = (pts.astype(np.float64) - np.array([-1.5, 0.25, -0.75])) / 0.125 - 0.5
    centre = u[:, 0::8][np.isfinite(u[:, 0::8]).all(-1)]
    assert np.array_equal(centre, np.rint(centre)) and np.isnan(pts).sum() == 1 and np.isinf(pts).sum() == 2
    fin = np.isfinite(u).all(-1)
    outside = ((u < 0) | (u > np.array([4, 2, 3]))).sum(-1)
    assert {1, 2, 3} <= set(outside[fin].tolist())


def test_sampler_gradient_against_central_differences():
    """``sample_ref``'s gradient against central differences of its value, h = 1e-6 voxel, at points whose u is more than 1e-3 away from
    every integer (and from the clamps).  Between integers the value is a polynomial of degree <= 3 in the point plus a Euclidean norm, so
    the differences' truncation error is ~h^2 and what remains is rounding: ~1e-16 * |value| / h.  Measured maximum over the cases
    below: 1.5e-9; the bound is 10 times that."""
    BOUND = 1.5e-8
    worst = 0.0
    for G, dim, signed in (((7, 6, 5), 3, False), ((7, 6, 5), 3, True), ((9, 1, 4), 3, True), ((12, 9, 1), 2, False)):
        N, P = 3, 200
        occ = DC.blob(G, N)
        occ[1] = 0  # a frame without a hull
        d_out = DR.edt_brute(occ, 0, 0)
        d_in = DR.edt_brute(occ, 1, 1) if signed else None
        origin = np.array([[-0.31, 0.12, 0.05], [0.2, -0.4, 0.1], [0.0, 0.0, 0.0]])
        voxel = np.array([0.11, 0.07, 1.0])
        pts = DC.sample_points(G, origin, voxel, N, P, dim, seed=3)
        pts = np.where(np.isfinite(pts), pts, np.float32(0.123))
        xyz = pts[..., ::-1] if dim == 2 else pts
        u = (xyz.astype(np.float64) - origin[:, None, :dim]) / voxel[:, None, None] - 0.5
        ext = np.array(G[:dim], np.float64)
        smooth = (np.abs(u - np.rint(u)) > 1e-3).all(-1)
        assert smooth.sum() >= 150  # (an axis with G = 1 has its kink at u = 0, where every point inside the grid lies)
        value, grad = DR.sample_ref(d_out, d_in, origin, voxel, pts, dim)
        assert np.isfinite(value).all() and (value[1] == voxel[1] * np.sqrt((np.maximum(np.maximum(-u[1], u[1] - (ext - 1)), 0) ** 2).sum(-1))).all()
        for a in range(dim):
            h = 1e-6 * voxel[:, None]
            # (float64 points: the reference takes float32 ones, so the differences are formed by shifting the origin instead)
            shift = np.zeros((N, 3))
            col = a if dim == 3 else 1 - a
            shift[:, col] = h[:, 0]
            hi, _ = DR.sample_ref(d_out, d_in, origin - shift, voxel, pts, dim)
            lo, _ = DR.sample_ref(d_out, d_in, origin + shift, voxel, pts, dim)
            err = np.abs((hi - lo) / (2 * h) - grad[..., a])[smooth]
            worst = max(worst, float(err.max()))
    print(f"sampler gradient against central differences: max error {worst:.3g}")
    assert worst <= BOUND


def test_sampler_closed_forms():
    """One occupied voxel in the middle of a 5^3 grid: at a cell centre the value is voxel * the cell's distance; a point outside the grid
    adds its distance to the box of centres; NONE reads 0; a NaN point reads 0."""
    occ = np.zeros((2, 5, 5, 5), np.uint8)
    occ[0, 2, 2, 2] = 1
    d = DR.edt_brute(occ, 0, 0)
    assert (d[1] == DR.NONE).all()
    origin, voxel = np.array([[-1.25, -1.25, -1.25]]), np.array([0.5])
    pts = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, -1.0], [2.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.25, 0.0, 0.0]]] * 2, np.float32)
    value, grad = DR.sample_ref(d, None, origin, voxel, pts, 3)
    assert np.allclose(value[0], [0.0, 1.0, np.sqrt(3.0), 1.0 + 1.0, 0.0, 0.25]) and (value[1] == [0, 0, 0, 1.0, 0, 0]).all()
    # y and z sit on the integer u = 2: the slope there is that of the cell to the right (2 -> 3), x is clamped (slope 0, unit pull)
    assert np.allclose(grad[0, 3], [1.0, np.sqrt(5.0) - 2.0, np.sqrt(5.0) - 2.0]) and (grad[0, 4] == 0).all()
    assert np.allclose(grad[0, 5], [1.0, 0.5 * np.sqrt(2.0), 0.5 * np.sqrt(2.0)])  # x halfway between the cells 2 and 3
    assert np.allclose(grad[1, 3], [1.0, 0.0, 0.0]) and (grad[1, :3] == 0).all()


# ---- the C ABI's argument validation (no GPU: every call fails before its first launch) -------------------------------------------
def _grid(lib_mod, N=1, G=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=(0.1,)):
    o = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(-1, 3))
    s = np.ascontiguousarray(np.asarray(voxel, np.float64).reshape(-1))
    g = lib_mod.HullGrid()
    g.N, (g.Gx, g.Gy, g.Gz) = N, G
    g.origin, g.n_origin, g.voxel_size, g.n_voxel_size = o.ctypes.data, o.shape[0], s.ctypes.data, s.shape[0]
    return g, (o, s)


def test_distance_field_argument_validation_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    assert b"0.9" in lib.smil_version() and b"distance fields" in lib.smil_version() and _lib.EDT_NONE == DR.NONE
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data  # a non-null stand-in: nothing is dereferenced before the arguments are accepted
    err = lambda: lib.smil_last_error()  # noqa: E731

    def edt(g, occ=p, d2=p, ws=p):
        return lib.smil_hull_edt(ctypes.byref(g), occ, 0, 0, d2, ws, None)

    def sample(g, dim=3, d2=p, pts=p, value=p, ws=p, P=5):
        return lib.smil_field_sample(ctypes.byref(g), d2, None, pts, dim, P, value, None, ws, None)

    g, keep = _grid(_lib)
    assert lib.smil_hull_edt(None, p, 0, 0, p, p, None) == -1 and b"null grid" in err(), err()
    for kw in (dict(occ=None), dict(d2=None), dict(ws=None)):
        assert edt(g, **kw) == -1 and b"null occ, d2 or workspace" in err(), err()
    for G in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        gb, kb = _grid(_lib, G=G)
        assert edt(gb) == -1 and b"below 1" in err(), err()
        assert sample(gb) == -1 and b"below 1" in err(), err()
        assert lib.smil_hull_edt_workspace_bytes(ctypes.byref(gb)) == 0
    gb, kb = _grid(_lib, N=0)
    assert edt(gb) == -1 and b"N=0" in err(), err()
    # (Gx+1)^2 + (Gy+1)^2 + (Gz+1)^2 >= 2^31 is refused: 46340^2 = 2^31 - 88 048, 46341^2 = 2^31 + 4 633
    for G, ok in (((46339, 1, 1), True), ((46340, 1, 1), False), ((32766, 32766, 100), True), ((32767, 32767, 2), False)):
        gb, kb = _grid(_lib, G=G)
        s = sum((x + 1) ** 2 for x in G)
        assert (s < 2**31) == ok
        if not ok:
            assert edt(gb) == -1 and b"exceed an int32" in err(), (G, err())
        else:  # accepted as far as the grid goes: the next check fails instead
            assert edt(gb, occ=None) == -1 and b"null occ" in err(), (G, err())
    # the workspace: 256 bytes unless a line leaves the LDS path, then a second int32 grid
    assert lib.smil_hull_edt_workspace_bytes(None) == 0 and lib.smil_hull_edt_workspace_bytes(ctypes.byref(g)) == 256
    for G, second in (((2, 3, DC.LDS_LINE), False), ((2, 3, DC.LDS_LINE + 1), True), ((128, DC.LDS_LINE + 1, 1), True), ((2, DC.LDS_LINE + 1, 1), False),
                      ((256, 256, 256), False)):
        gb, kb = _grid(_lib, N=2, G=G)
        want = -(-2 * G[0] * G[1] * G[2] * 4 // 256) * 256 if second else 256
        assert lib.smil_hull_edt_workspace_bytes(ctypes.byref(gb)) == want, G
    # the sampler
    for dim in (1, 4, 0):
        assert sample(g, dim=dim) == -1 and b"outside {2, 3}" in err(), err()
    assert sample(g, dim=2) == -1 and b"needs Gz=1" in err(), err()
    g2, keep2 = _grid(_lib, G=(4, 4, 1))
    assert sample(g2, dim=2, d2=None) == -1 and b"null d2_out" in err(), err()
    for kw in (dict(d2=None), dict(pts=None), dict(value=None), dict(ws=None)):
        assert sample(g, **kw) == -1 and b"null d2_out, points, value or workspace" in err(), err()
    assert sample(g, P=-1) == -1 and b"P=-1" in err(), err()
    for voxel in (0.0, -0.1, float("nan"), float("inf")):
        gb, kb = _grid(_lib, voxel=(voxel,))
        assert sample(gb) == -1 and b"must be positive and finite" in err(), err()
    gb, kb = _grid(_lib, origin=(0.0, float("inf"), 0.0))
    assert sample(gb) == -1 and b"must be finite" in err(), err()
    gb, kb = _grid(_lib, N=3, origin=np.zeros((2, 3)))
    assert sample(gb) == -1 and b"origin has 2 rows" in err(), err()
    gb, kb = _grid(_lib, N=3, voxel=(0.1, 0.1))
    assert sample(gb) == -1 and b"voxel_size has 2 rows" in err(), err()
    gb, kb = _grid(_lib)
    gb.origin = None
    assert sample(gb) == -1 and b"null origin or voxel_size" in err(), err()
