"""GPU tests of the visual hull (``pytest -m gpu``): ``visual_hull.carve`` / ``query_points`` / ``VisualHull`` against the numpy float64
restatement (tests/visual_hull_ref.py) on the seeded cases of tests/visual_hull_cases.py.

Conditions.  ``occ``, ``fg``, ``seen`` equal the restatement's wherever its bounds coincide (no ambiguous (point, view) pair touches the voxel)
and lie within the bounds elsewhere (tests/test_visual_hull_cpu.py caps the ambiguous voxels of every case at 1e-4); ``occ`` is the vote
rule of the GPU's own counts everywhere.  The statistics are bit-equal to the restatement's recomputed from the GPU's own ``occ``; so is
the surface, points (as bits) and order.  Two calls give the same bits.  Shapes: Gx in {1, 63, 64, 65} x Gy, Gz in {1, 3, 5} and (65, 3, 2);
1, 2, 63, 64 views (65 raises); N in {1, 2, 3} with an all-background frame in the middle; camera tables of 1, views and N * views rows with and
without aspect_ratio / principal_point; uint8, bool and float32 masks (threshold, a NaN pixel), 48 x 80 and 1 x 1; points behind a camera
and outside the image with outside_carves off and on; seen = min_views - 1 and = min_views, max_misses 0 and 1; per-frame against shared
origin and voxel size; one call beyond 2^31 voxels.
"""
import numpy as np
import pytest
import torch

import visual_hull_cases as VC
import visual_hull_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cams(c):
    return {k: torch.from_numpy(v) for k, v in c.cams.items()}


def _carve(c, masks=None, **over):
    from smilify_amd import visual_hull as VH

    masks = torch.from_numpy(c.masks).to(DEV) if masks is None else masks
    args = dict(image_size=c.S, origin=c.origin, voxel_size=c.voxel_size, grid=c.grid, min_views=c.min_views, max_misses=c.max_misses,
                outside_carves=c.outside_carves, threshold=c.threshold, return_counts=True)
    args.update(over)
    return VH.carve(masks, _cams(c), **args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(c, hull, ref, origin=None, voxel_size=None):
    """The conditions of the module docstring for one carve; returns the GPU's occ."""
    origin = c.origin if origin is None else origin
    voxel_size = c.voxel_size if voxel_size is None else voxel_size
    occ_ref, v = ref
    Gx, Gy, Gz = c.grid
    occ, fg, seen = (t.cpu().numpy() for t in (hull.occupancy, hull.fg, hull.seen))
    assert occ.shape == fg.shape == seen.shape == (c.N, Gz, Gy, Gx) and occ.dtype == fg.dtype == seen.dtype == np.uint8
    e = v.exact
    print(f"{c.name}: {occ.size} voxels, {int((~e).sum())} ambiguous, {int(occ.sum())} occupied")
    assert np.array_equal(fg[e], v.fg[e]) and np.array_equal(seen[e], v.seen[e]) and np.array_equal(occ[e], occ_ref[e])
    assert (fg >= v.fg_lo).all() and (fg <= v.fg_hi).all() and (seen >= v.seen_lo).all() and (seen <= v.seen_hi).all()
    assert np.array_equal(occ, VR.occupancy_rule(fg.astype(np.int64), seen.astype(np.int64), c.min_views, c.max_misses))
    # statistics and surface from the GPU's own occ: bit-equal
    assert np.array_equal(hull._raw_stats().cpu().numpy(), VR.stats(occ))
    pts, idx, off = hull.surface_points(return_index=True)
    r_pts, r_idx, r_off = VR.surface(occ, origin, voxel_size)
    assert pts.dtype == torch.float32 and idx.dtype == off.dtype == torch.int64 and tuple(pts.shape) == (len(r_idx), 3)
    assert np.array_equal(off.cpu().numpy(), r_off) and np.array_equal(idx.cpu().numpy(), r_idx)
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(r_pts))
    pts2, off2 = hull.surface_points()
    assert torch.equal(pts2, pts) and torch.equal(off2, off)
    return occ


@pytest.mark.parametrize("name", VC.SMALL_CASES)
def test_carve_against_the_restatement(name):
    c = VC.get(name)
    masks = torch.from_numpy(c.masks).to(DEV)
    assert masks.dtype == {"mask_bool": torch.bool, "mask_f32_nan": torch.float32}.get(name, torch.uint8)
    hull = _carve(c, masks)
    _check(c, hull, VC.reference(name))
    again = _carve(c, masks)  # two calls: the same bits
    for a, b in ((hull.occupancy, again.occupancy), (hull.fg, again.fg), (hull.seen, again.seen)):
        assert torch.equal(a, b)
    plain = _carve(c, masks, return_counts=False)  # without the counts: the same occupancy
    assert plain.fg is None and plain.seen is None and torch.equal(plain.occupancy, hull.occupancy)


@pytest.mark.parametrize("Gx", VC.GRID_GX)
def test_grid_shapes(Gx):
    """Gx x (Gy, Gz in {1, 3, 5}): three frames, the middle one empty - in ``offsets`` and in the statistics too."""
    for name in (n for n in VC.GRID_CASES if n.startswith(f"grid_{Gx}_")):
        c = VC.get(name)
        hull = _carve(c)
        occ = _check(c, hull, VC.reference(name))
        st = hull.stats()
        _, off = hull.surface_points()
        assert occ[1].sum() == 0 and int(st.count[1]) == 0 and int(off[1]) == int(off[2])
        assert st.index_min[1].tolist() == list(c.grid) and st.index_max[1].tolist() == [-1, -1, -1]


def test_65_views_raise():
    from smilify_amd import _lib, engine
    from smilify_amd import visual_hull as VH

    c = VC.get("views_64")
    masks = torch.zeros(1, 65, c.H, c.W, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.SmilError, match="outside 1..64"):
        VH.carve(masks, _cams(c), image_size=c.S, origin=c.origin, voxel_size=c.voxel_size, grid=c.grid)
    with pytest.raises(_lib.SmilError, match="outside 1..64"):
        VH.query_points(torch.zeros(1, 4, 3), masks, _cams(c), image_size=c.S)
    cams = engine.CameraSet(*(torch.from_numpy(c.cams[k][:1]).to(DEV) for k in ("R", "T")), torch.from_numpy(c.cams["fov"]).to(DEV), None, 65, c.S)
    with pytest.raises(_lib.SmilError, match="views=65 outside 1..64"):  # the library's own check
        engine.hull_carve(engine.HullGridSpec(1, c.grid, c.origin, c.voxel_size), masks, cams, 1, 0)
    with pytest.raises(_lib.SmilError, match="positive and finite"):
        _carve(c, voxel_size=0.0)
    with pytest.raises(_lib.SmilError, match="min_views=65"):
        _carve(c, min_views=65)


@pytest.mark.parametrize("name", ["dyadic_0", "dyadic_1", "mask_f32_nan"])
def test_query_points_reproduce_the_carve(name):
    """The voxel centres of these grids are float32 numbers (dyadic origin and voxel size; mask_f32_nan: compared through the
    restatement at the rounded centres instead), so ``query_points`` at them tests the very points the carve tested."""
    from smilify_amd import visual_hull as VH

    c = VC.get(name)
    masks = torch.from_numpy(c.masks).to(DEV)
    hull = _carve(c, masks)
    centres = VR.centres(c.N, c.origin, c.voxel_size, c.grid)
    pts32 = centres.astype(np.float32)
    fg, seen = VH.query_points(torch.from_numpy(pts32).to(DEV), masks, _cams(c), image_size=c.S, threshold=c.threshold,
                               outside_carves=c.outside_carves)
    assert fg.dtype == seen.dtype == torch.uint8 and tuple(fg.shape) == (c.N, centres.shape[1])
    if name.startswith("dyadic"):
        assert np.array_equal(pts32.astype(np.float64), centres)
        assert torch.equal(fg.reshape(hull.fg.shape), hull.fg) and torch.equal(seen.reshape(hull.seen.shape), hull.seen)
    v = VR.votes(pts32.astype(np.float64), c.masks, c.cams, c.S, c.threshold, c.outside_carves)
    e = v.exact
    assert e.mean() >= 1.0 - VC.AMBIGUOUS_CAP
    assert np.array_equal(fg.cpu().numpy()[e], v.fg[e]) and np.array_equal(seen.cpu().numpy()[e], v.seen[e])
    fg2, seen2 = VH.query_points(torch.from_numpy(pts32).to(DEV), masks, _cams(c), image_size=c.S, threshold=c.threshold,
                                 outside_carves=c.outside_carves)
    assert torch.equal(fg, fg2) and torch.equal(seen, seen2)


def test_shared_against_per_frame_tables():
    """One row of origin / voxel size for every frame, and the same row repeated per frame: the same bits."""
    c = VC.get("rows_views")
    shared = _carve(c)
    per_frame = _carve(c, origin=np.repeat(c.origin, c.N, axis=0), voxel_size=np.repeat(c.voxel_size, c.N))
    assert tuple(per_frame.origin.shape) == (c.N, 3) and tuple(shared.origin.shape) == (1, 3)
    for a, b in ((shared.occupancy, per_frame.occupancy), (shared.fg, per_frame.fg), (shared.seen, per_frame.seen)):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(shared.surface_points(True), per_frame.surface_points(True)))


def test_stats_and_sample_surface():
    """``stats()`` against the moments of the restatement's integer sums; an empty frame gives NaN rows and zero samples; every sample of
    ``sample_surface`` is a row of ``surface_points`` of its own frame."""
    c = VC.get("per_frame")
    hull = _carve(c)
    occ = hull.occupancy.cpu().numpy()
    st = hull.stats()
    count, centroid, cov = VR.moments(VR.stats(occ), c.origin, c.voxel_size)
    assert st.centroid.dtype == st.covariance.dtype == torch.float64 and tuple(st.covariance.shape) == (c.N, 3, 3)
    assert np.array_equal(st.count.cpu().numpy(), count) and count[1] == 0 and count[0] > 0 and count[2] > 0
    assert np.isnan(st.centroid[1].cpu().numpy()).all() and np.isnan(st.covariance[1].cpu().numpy()).all()
    full = [0, 2]
    # float64 on both sides, the same few operations: 1e-12 relative to the grid's extent (squared) leaves room for their order only
    extent = float(max(c.grid) * c.voxel_size.max())
    assert np.abs(st.centroid.cpu().numpy()[full] - centroid[full]).max() <= 1e-12 * extent
    assert np.abs(st.covariance.cpu().numpy()[full] - cov[full]).max() <= 1e-12 * extent * extent
    S = 50
    pts, off = hull.surface_points()
    sample = hull.sample_surface(S, seed=3)
    assert tuple(sample.shape) == (c.N, S, 3) and sample.dtype == torch.float32 and torch.equal(sample, hull.sample_surface(S, seed=3))
    assert not torch.equal(sample, hull.sample_surface(S, seed=4))
    pts, off, sample = pts.cpu().numpy(), off.cpu().numpy(), sample.cpu().numpy()
    assert (sample[1] == 0).all() and off[1] == off[2]
    for n in full:
        rows = {r.tobytes() for r in pts[off[n]:off[n + 1]]}
        assert len(rows) > 3 and all(r.tobytes() in rows for r in sample[n])
        assert len({r.tobytes() for r in sample[n]}) > 3


@pytest.mark.parametrize("N, grid", [(6, (64, 64, 52)), (4, (64, 64, 64))])
def test_surface_offsets_across_scan_rounds(N, grid):
    """The scan of the per-workgroup surface counts takes 1 024 counts a round (a workgroup counts 1 024 voxels).  6 frames of 64 x 64 x 52:
    208 counts a frame, 1 248 in all - frame 5 starts at count 1 040, inside the second round, whose prefixes carry the first round's
    total.  4 frames of 64^3: exactly 1 024 counts, one full round.  Occupancy built directly (``scan_occupancy``: frame 2 empty)."""
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH

    Gx, Gy, Gz = grid
    counts = N * -(-Gx * Gy * Gz // 1024)
    assert counts == (1248 if N == 6 else 1024)
    occ = VC.scan_occupancy(N, grid)
    origin, voxel = np.array([[-1.5, 0.25, -0.75]]), np.array([0.125])
    hull = VH.VisualHull(torch.from_numpy(occ).to(DEV), None, None, engine.HullGridSpec(N, grid, origin, voxel))
    pts, idx, off = hull.surface_points(True)
    r_pts, r_idx, r_off = VR.surface(occ, origin, voxel)
    assert r_off[2] == r_off[3] and (np.diff(r_off)[[0, 1, *range(3, N)]] > 100).all()
    assert np.array_equal(off.cpu().numpy(), r_off) and np.array_equal(idx.cpu().numpy(), r_idx)
    assert tuple(pts.shape) == (len(r_idx), 3) and np.array_equal(_bits(pts.cpu().numpy()), _bits(r_pts))


def test_tight_bounds_second_pass():
    """Coarse to fine: the grid of ``tight_bounds`` holds the voxel of every coarse occupied centre, is finer, and the second carve agrees
    with the restatement on it."""
    c = VC.get("two_ellipsoids")
    masks = torch.from_numpy(c.masks).to(DEV)
    coarse = _carve(c, masks)
    origin, voxel = coarse.tight_bounds(margin_voxels=1)
    assert origin.dtype == voxel.dtype == torch.float64 and tuple(origin.shape) == (c.N, 3) and tuple(voxel.shape) == (c.N,)
    origin, voxel = origin.cpu().numpy(), voxel.cpu().numpy()
    assert (voxel < c.voxel_size[0]).all() and (voxel > 0.3 * c.voxel_size[0]).all()
    centres = VR.centres(c.N, c.origin, c.voxel_size, c.grid)
    occ = coarse.occupancy.cpu().numpy().reshape(c.N, -1).astype(bool)
    half = 0.5 * c.voxel_size[0]
    for n in range(c.N):
        X = centres[n][occ[n]]
        assert len(X) > 100
        assert (X - half >= origin[n] - 1e-12).all() and (X + half <= origin[n] + np.array(c.grid) * voxel[n] + 1e-12).all()
    fine = _carve(c, masks, origin=origin, voxel_size=voxel)
    ref = VR.carve(c.masks, c.cams, c.S, origin, voxel, c.grid, c.min_views, c.max_misses, c.outside_carves, c.threshold)
    assert 1.0 - ref[1].exact.mean() <= VC.AMBIGUOUS_CAP
    _check(c, fine, ref, origin, voxel)
    assert fine.occupancy.sum() > coarse.occupancy.sum()  # the same hull in smaller voxels


def test_beyond_2_31_voxels():
    """N = 2 frames of 1100 x 1000 x 1000 voxels, one view, occ only (2.2 GB): checked at 100 000 seeded voxel indices - a third of them
    in the part of frame 1 whose global index exceeds 2^31 - through the restatement's point query."""
    from smilify_amd import visual_hull as VH

    c = VC.big_case()
    Gx, Gy, Gz = c.grid
    vox = Gx * Gy * Gz
    assert c.N * vox > 2**31
    masks = torch.from_numpy(c.masks).to(DEV)
    hull = VH.carve(masks, _cams(c), image_size=c.S, origin=c.origin, voxel_size=c.voxel_size, grid=c.grid, min_views=1)
    occ = hull.occupancy
    assert tuple(occ.shape) == (2, Gz, Gy, Gx) and hull.fg is None
    rng = np.random.default_rng(c.cams["R"].shape[0] + 71)
    M = 100_000
    frame = rng.integers(0, 2, M)
    linear = rng.integers(0, vox, M)
    frame[: M // 3] = 1
    linear[: M // 3] = rng.integers(2**31 - vox, vox, M // 3)  # global index frame * vox + linear >= 2^31
    linear[-4:] = [0, vox - 1, 0, vox - 1]
    frame[-4:] = [0, 0, 1, 1]
    got = occ.reshape(-1)[torch.from_numpy(frame * vox + linear).to(DEV)].cpu().numpy()
    pts = VR.points_at(linear, frame, c.origin, c.voxel_size, c.grid)
    want = np.zeros(M, np.uint8)
    exact = np.zeros(M, bool)
    for f in range(2):
        sel = frame == f
        v = VR.votes(pts[sel][None], c.masks[f:f + 1], {k: (t[f:f + 1] if t.shape[0] == 2 else t) for k, t in c.cams.items()}, c.S)
        want[sel] = VR.occupancy_rule(v.fg[0], v.seen[0], 1, 0)
        exact[sel] = v.exact[0]
    tail = (frame * vox + linear) >= 2**31
    print(f"big: {int(exact.sum())} of {M} exact, {int(want.sum())} occupied, {int(want[tail].sum())} of {int(tail.sum())} beyond 2^31")
    assert exact.mean() >= 1.0 - VC.AMBIGUOUS_CAP and tail.sum() >= M // 3
    assert 0 < want[tail].sum() < tail.sum() and 0 < want[~tail].sum() < (~tail).sum()
    assert np.array_equal(got[exact], want[exact])


def test_hull_of_the_librarys_own_pictures(tables):
    """The synthetic model posed, rendered in 6 views at 64^2 by ``Renderer.render_fragments``; masks = face id >= 0.  The carve agrees with
    the restatement on those masks, and every posed vertex is seen by all 6 views."""
    from smilify_amd import engine, synthetic
    from smilify_amd import visual_hull as VH
    from smilify_amd.p3d_renderer import Renderer

    t = tables("synthetic")
    S, views = 64, 6
    dm = engine.DeviceModel(t, DEV)
    pose, trans = synthetic.random_pose(1, t.J, torch.Generator().manual_seed(5))
    out = engine.lbs_forward(dm, torch.zeros(t.nB, device=DEV), pose.to(DEV).contiguous(), trans=trans.to(DEV).contiguous(), shared_beta=True,
                             trans_after_joints=True)
    verts = out["verts"]
    R, T = synthetic.camera_ring(views, 2.7)
    fov = torch.full((1,), 60.0)
    r = Renderer(S, DEV, views=views)
    r.set_camera_parameters(R, T, fov)
    faces = torch.from_numpy(t.faces.astype(np.int64)).to(DEV)[None]
    masks = (r.render_fragments(verts, faces, want=("pix_to_face",)).pix_to_face >= 0).reshape(1, views, S, S)
    assert masks.dtype == torch.bool and masks.any()
    cams = dict(R=R, T=T, fov=fov)
    fg, seen = VH.query_points(verts, masks, cams, image_size=S)
    assert (seen == views).all()
    lo, hi = verts[0].min(0).values.cpu().numpy().astype(np.float64), verts[0].max(0).values.cpu().numpy().astype(np.float64)
    grid = (24, 24, 24)
    voxel = float((hi - lo).max()) * 1.1317 / 24
    origin = 0.5 * (lo + hi) - 12 * voxel + np.array([0.0037, -0.0021, 0.0043])
    hull = VH.carve(masks, cams, image_size=S, origin=origin, voxel_size=voxel, grid=grid, min_views=views, return_counts=True)
    c = VC.SimpleNamespace(name="rendered", N=1, grid=grid, origin=origin.reshape(1, 3), voxel_size=np.array([voxel]), min_views=views, max_misses=0)
    ref = VR.carve(masks.cpu().numpy(), {k: v.numpy() for k, v in cams.items()}, S, origin, voxel, grid, views)
    assert 1.0 - ref[1].exact.mean() <= VC.AMBIGUOUS_CAP
    occ = _check(c, hull, ref)
    assert occ.sum() > 50
    centroid = hull.stats().centroid[0].cpu().numpy()
    assert (centroid > lo).all() and (centroid < hi).all()
