"""CPU checks of the visual hull (no GPU): the numpy restatement (tests/visual_hull_ref.py) against first principles on the analytic scenes
of tests/visual_hull_cases.py, the cap on ambiguous voxels every case must keep, that the cases hold what the GPU tests say they exercise,
and the argument validation of the C ABI through ctypes.

First principles, for an ellipsoid E (centre c, radii r) every view sees whole, masks computed per pixel centre:
 * a voxel centre inside E shrunk by 0.9 is occupied: the centre of the pixel it projects into lies at most sqrt(1/2) pixel away, so that
   pixel's ray passes within 1.5 pixel footprints z / (S/2 k) of the point - inside E when 0.1 min(r) covers that, which the test checks;
 * no occupied centre lies outside the outlines: the ray from any camera through an occupied centre meets E grown by 1 / 0.9 (the same
   margin, the other way round);
 * the hull's centroid lies within one voxel of c (the rig surrounds the ellipsoid).
"""
import ctypes

import numpy as np
import pytest

import visual_hull_cases as VC
import visual_hull_ref as VR


def _inside(points, ellipsoids, scale):
    return np.any([(((points - c) / (r * scale)) ** 2).sum(-1) <= 1.0 for c, r in ellipsoids], axis=0)


def _footprint(c):
    """The largest pixel footprint (world units per pixel at the depth of a voxel centre) over the case's voxels and views."""
    pts = VR.centres(c.N, c.origin, c.voxel_size, c.grid)
    _, _, z = VR.project(pts, c.cams, c.S, c.views)
    _, _, k00, k11, _ = VR.camera_tables(c.cams, c.N, c.views)
    inside = _inside(pts, c.ellipsoids, 1.0 / 0.9)
    zmax = np.where(inside[:, None, :], z, 0.0).max(axis=2).reshape(-1)  # (images) the deepest point that matters
    return float((zmax / (0.5 * c.S * np.minimum(k00, k11))).max())


@pytest.mark.parametrize("name", ["ellipsoid32", "two_ellipsoids"])
def test_restatement_against_the_analytic_ellipsoids(name):
    c = VC.get(name)
    occ, v = VC.reference(name)
    pts = VR.centres(c.N, c.origin, c.voxel_size, c.grid)
    occ_flat = occ.reshape(c.N, -1).astype(bool)
    fp = _footprint(c)
    r_min = min(float(r.min()) for _, r in c.ellipsoids)
    assert 0.1 * r_min >= 1.5 * fp, (r_min, fp)  # the factor 0.9 covers the pixel footprint
    shrunk = _inside(pts, c.ellipsoids, 0.9)
    assert shrunk.sum() > 500 and occ_flat[shrunk].all()
    # every occupied centre's ray meets the grown ellipsoid(s) in every view
    R, T, _, _, _ = VR.camera_tables(c.cams, c.N, c.views)
    for n in range(c.N):
        X = pts[n][occ_flat[n]]
        assert len(X) > 500
        for view in range(c.views):
            Rinv = np.linalg.inv(R[n * c.views + view])
            C = -T[n * c.views + view] @ Rinv
            hit = np.zeros(len(X), bool)
            for centre, radii in c.ellipsoids:
                p, q = (C - centre) / (radii / 0.9), (X - C) / (radii / 0.9)
                a, b, cc = (q * q).sum(-1), 2.0 * (q * p).sum(-1), (p * p).sum() - 1.0
                hit |= b * b - 4.0 * a * cc >= 0.0
            assert hit.all(), (n, view, int((~hit).sum()))
    if len(c.ellipsoids) == 1:
        count, centroid, cov = VR.moments(VR.stats(occ), c.origin, c.voxel_size)
        err = np.abs(centroid - c.ellipsoids[0][0]).max()
        print(f"{name}: {int(count[0])} occupied voxels, centroid off by {err:.4f} (voxel {c.voxel_size[0]})")
        assert err <= c.voxel_size[0]
        assert (np.linalg.eigvalsh(cov[0]) > 0).all()


@pytest.mark.parametrize("G", [(1, 1, 1), (2, 2, 2), (7, 7, 7), (65, 3, 2), (9, 1, 4)])
def test_full_grid_closed_forms(G):
    Gx, Gy, Gz = G
    occ = np.ones((2, Gz, Gy, Gx), np.uint8)
    occ[1] = 0
    st = VR.stats(occ)
    n = Gx * Gy * Gz
    s1 = lambda g: g * (g - 1) // 2  # noqa: E731
    s2 = lambda g: (g - 1) * g * (2 * g - 1) // 6  # noqa: E731
    want = [n, s1(Gx) * Gy * Gz, s1(Gy) * Gx * Gz, s1(Gz) * Gx * Gy, s2(Gx) * Gy * Gz, s2(Gy) * Gx * Gz, s2(Gz) * Gx * Gy,
            s1(Gx) * s1(Gy) * Gz, s1(Gx) * s1(Gz) * Gy, s1(Gy) * s1(Gz) * Gx, 0, 0, 0, Gx - 1, Gy - 1, Gz - 1]
    assert st[0].tolist() == want
    assert st[1].tolist() == [0] * 10 + [Gx, Gy, Gz, -1, -1, -1]
    pts, idx, off = VR.surface(occ, (0.1, 0.2, 0.3), 0.5)
    inner = max(Gx - 2, 0) * max(Gy - 2, 0) * max(Gz - 2, 0)
    assert off.tolist() == [0, n - inner, n - inner] and len(pts) == len(idx) == n - inner  # G^3 - (G - 2)^3 for a cube
    assert (np.diff(idx) > 0).all() and pts.dtype == np.float32
    count, centroid, cov = VR.moments(st, (0.1, 0.2, 0.3), 0.5)
    assert np.allclose(centroid[0], np.array([0.1, 0.2, 0.3]) + 0.25 * np.array(G)) and np.isnan(centroid[1]).all() and np.isnan(cov[1]).all()
    assert np.allclose(np.diag(cov[0]), 0.25 * (np.array(G, float) ** 2 - 1) / 12.0) and abs(cov[0][0, 1]) < 1e-12


@pytest.mark.parametrize("name", VC.SMALL_CASES + ["grids"])
def test_cases_keep_the_ambiguity_cap(name):
    names = VC.GRID_CASES if name == "grids" else [name]
    for n in names:
        frac = VC.ambiguous_fraction(n)
        assert frac <= VC.AMBIGUOUS_CAP, (n, frac)
        occ, v = VC.reference(n)
        assert (v.fg_lo <= v.fg).all() and (v.fg <= v.fg_hi).all() and (v.seen_lo <= v.seen).all() and (v.seen <= v.seen_hi).all()
        assert (v.fg <= v.seen).all() and v.seen.max() <= VC.get(n).views


def test_cases_hold_what_they_are_for():
    """The GPU tests lean on these properties of the seeded cases."""
    for n in VC.GRID_CASES + ["per_frame"]:  # an empty frame between full ones (where the grid reaches the ellipsoid at all)
        occ, _ = VC.reference(n)
        assert occ[1].sum() == 0, n
    assert sum(VC.reference(n)[0][0].any() and VC.reference(n)[0][2].any() for n in VC.GRID_CASES) >= 20
    c = VC.get("outside_0")
    ys, xs, z = VR.project(VR.centres(c.N, c.origin, c.voxel_size, c.grid), c.cams, c.S, c.views)
    front = z > VR.ZNEAR
    inside = front & (ys >= 0) & (ys < c.H) & (xs >= 0) & (xs < c.W)
    assert (~front).sum() > 10 and (front & ~inside).sum() > 10 and inside.sum() > 10  # behind a camera, outside the image, seen
    off, on = VC.reference("outside_0"), VC.reference("outside_1")
    assert (off[0] != on[0]).any() and (on[1].seen >= off[1].seen).all() and (on[1].fg == off[1].fg).all()
    for m in (0, 1):  # the vote rule's threshold from both sides, and misses that max_misses = 1 forgives
        c = VC.get(f"votes_m{m}")
        occ, v = VC.reference(f"votes_m{m}")
        assert (v.seen == c.min_views - 1).sum() > 10 and (v.seen == c.min_views).sum() > 10
        assert ((v.seen >= c.min_views) & (v.seen - v.fg == 1)).sum() > 10
    assert VC.reference("votes_m1")[0].sum() > VC.reference("votes_m0")[0].sum()
    c = VC.get("mask_f32_nan")  # the NaN pixel is looked up, and counts as background
    assert np.isnan(c.masks).sum() == 1
    clean = np.where(np.isnan(c.masks), np.float32(0.8), c.masks)
    _, v_clean = VR.carve(clean, c.cams, c.S, c.origin, c.voxel_size, c.grid, c.min_views, c.max_misses, c.outside_carves, c.threshold)
    assert (v_clean.fg != VC.reference("mask_f32_nan")[1].fg).any()
    c = VC.get("mask_1x1")
    assert c.masks.shape[2:] == (1, 1) and VC.reference("mask_1x1")[0].any() and not VC.reference("mask_1x1")[0].all()
    for n, rows in (("rows_one", 1), ("rows_views", 3), ("rows_images", 6)):
        assert VC.get(n).cams["R"].shape[0] == rows and "aspect_ratio" not in VC.get(n).cams
        assert VC.get(n + "_ap").cams["principal_point"].shape == (VC.get(n + "_ap").N * VC.get(n + "_ap").views, 2)


# ---- the C ABI's argument validation (no GPU: every call fails before its first launch) -------------------------------------------
def _grid(lib_mod, N=1, G=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=(0.1,)):
    o = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(-1, 3))
    s = np.ascontiguousarray(np.asarray(voxel, np.float64).reshape(-1))
    g = lib_mod.HullGrid()
    g.N, (g.Gx, g.Gy, g.Gz) = N, G
    g.origin, g.n_origin, g.voxel_size, g.n_voxel_size = o.ctypes.data, o.shape[0], s.ctypes.data, s.shape[0]
    return g, (o, s)


def _cameras(lib_mod, N, views, rows=None):
    rows = rows or views
    keep = [np.zeros((rows, 9), np.float32), np.zeros((rows, 3), np.float32), np.full(rows, 30.0, np.float32)]
    c = lib_mod.Cameras()
    c.N, c.views, c.S = N * views, views, 64
    c.R, c.nR, c.T, c.nT, c.fov, c.nFov = keep[0].ctypes.data, rows, keep[1].ctypes.data, rows, keep[2].ctypes.data, rows
    return c, keep


def test_hull_argument_validation_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    assert b"0.8" in lib.smil_version() and b"visual hull" in lib.smil_version()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data  # a non-null stand-in: nothing is dereferenced before the arguments are accepted
    err = lambda: lib.smil_last_error()  # noqa: E731

    def carve(g, cam, min_views=1, max_misses=0, masks=p, occ=p, ws=p, H=4, W=4, thr=0.0):
        return lib.smil_hull_carve(ctypes.byref(g), masks, 0, H, W, thr, ctypes.byref(cam), min_views, max_misses, 0, occ, None, None, ws, None)

    g, keep = _grid(_lib)
    for views in (0, 65):
        cam, k2 = _cameras(_lib, 1, views, rows=1)
        assert carve(g, cam) == -1 and b"views=%d outside 1..64" % views in err(), err()
    cam, k2 = _cameras(_lib, 1, 2)
    cam.N = 3
    assert carve(g, cam) == -1 and b"cameras hold N=3 images" in err(), err()
    cam, k2 = _cameras(_lib, 2, 4, rows=3)
    g2, keep2 = _grid(_lib, N=2)
    assert carve(g2, cam) == -1 and b"camera table R has 3 rows" in err(), err()
    cam, k2 = _cameras(_lib, 1, 2)
    for voxel in (0.0, -0.1, float("nan"), float("inf")):
        gb, kb = _grid(_lib, voxel=(voxel,))
        assert carve(gb, cam) == -1 and b"must be positive and finite" in err(), err()
    gb, kb = _grid(_lib, origin=(0.0, float("inf"), 0.0))
    assert carve(gb, cam) == -1 and b"must be finite" in err(), err()
    for G in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        gb, kb = _grid(_lib, G=G)
        assert carve(gb, cam) == -1 and b"below 1" in err(), err()
        assert lib.smil_hull_stats(ctypes.byref(gb), p, p, None) == -1 and b"below 1" in err()
        assert lib.smil_hull_surface_count(ctypes.byref(gb), p, p, p, None) == -1 and b"below 1" in err()
        assert lib.smil_hull_surface_workspace_bytes(ctypes.byref(gb)) == 0
    gb, kb = _grid(_lib, G=(1 << 20, 1 << 20, 2))
    assert carve(gb, cam) == -1 and b"2^40" in err(), err()
    gb, kb = _grid(_lib, N=3, origin=np.zeros((2, 3)))
    assert carve(gb, cam) == -1 and b"origin has 2 rows" in err(), err()
    gb, kb = _grid(_lib, N=3, voxel=(0.1, 0.1))
    assert carve(gb, cam) == -1 and b"voxel_size has 2 rows" in err(), err()
    gb, kb = _grid(_lib, N=0)
    assert carve(gb, cam) == -1 and b"N=0" in err(), err()
    for mv in (-1, 3):
        assert carve(g, cam, min_views=mv) == -1 and b"min_views" in err(), err()
    assert carve(g, cam, max_misses=-1) == -1 and b"max_misses" in err(), err()
    assert carve(g, cam, thr=float("nan")) == -1 and b"threshold" in err(), err()
    assert carve(g, cam, H=0) == -1 and b"masks of 0 x 4" in err(), err()
    assert carve(g, cam, masks=None) == -1 and b"null masks" in err(), err()
    assert carve(g, cam, occ=None) == -1 and b"null occ" in err(), err()
    assert carve(g, cam, ws=None) == -1 and b"null occ or workspace" in err(), err()
    assert lib.smil_hull_carve(None, p, 0, 4, 4, 0.0, ctypes.byref(cam), 1, 0, 0, p, None, None, p, None) == -1 and b"null grid" in err()
    # the other entry points
    assert lib.smil_hull_query(p, 1, 5, p, 0, 4, 4, 0.0, ctypes.byref(cam), 0, None, p, None) == -1 and b"null argument" in err(), err()
    assert lib.smil_hull_query(p, 0, 5, p, 0, 4, 4, 0.0, ctypes.byref(cam), 0, p, p, None) == -1 and b"bad sizes" in err(), err()
    cam65, k3 = _cameras(_lib, 1, 65, rows=1)
    assert lib.smil_hull_query(p, 1, 5, p, 0, 4, 4, 0.0, ctypes.byref(cam65), 0, p, p, None) == -1 and b"outside 1..64" in err(), err()
    assert lib.smil_hull_stats(ctypes.byref(g), None, p, None) == -1 and b"null argument" in err(), err()
    assert lib.smil_hull_surface_count(ctypes.byref(g), p, None, p, None) == -1 and b"null argument" in err(), err()
    assert lib.smil_hull_surface_write(ctypes.byref(g), p, p, None, None, None) == -1 and b"null argument" in err(), err()
    gb, kb = _grid(_lib, voxel=(0.0,))
    assert lib.smil_hull_surface_write(ctypes.byref(gb), p, p, p, None, None) == -1 and b"positive and finite" in err(), err()
    assert lib.smil_hull_carve_workspace_bytes(ctypes.byref(g)) >= 32 and lib.smil_hull_carve_workspace_bytes(None) == 0
    # one block of 1024 voxels: one int64 count, the origin, the voxel size - three regions
    assert lib.smil_hull_surface_workspace_bytes(ctypes.byref(g)) == 3 * 256
