"""GPU tests of the distance fields (``pytest -m gpu``): ``VisualHull.distance_transform`` / ``imageprep.mask_distance_transform`` against
``edt_brute`` (tests/distance_field_ref.py), bit for bit, and ``HullDistanceField.sample`` / ``imageprep.sample_mask_distance`` against
``sample_ref`` rounded once to float32.

Conditions.  Every ``d2`` equals the reference's as integers; two calls give the same bits.  Shapes: Gx in {1, 2, 63, 64, 65, 130} x Gy, Gz
in {1, 3, 5}, (3, 65, 2), (2, 3, 130), and one grid per further path of the kernel (tests/distance_field_cases.py, ``PATH_SHAPES``: among
them a z line and a y line of ``LDS_LINE + 1`` = 513 cells, one beyond the longest line the LDS path holds).  Patterns: a voxel in each of the
8 corners, two opposite corners, a plane, a checkerboard, random at 0.5 and 0.01, a full frame, an empty frame between two full ones, each
with ``invert`` and ``border`` off and on (all four combinations).  One call beyond 2^31 voxels.

The sampler.  The kernel performs the reference's float64 operations in the reference's order (no contraction), and sqrt and division
are correctly rounded on both sides, so one rounding to float32 is the whole expected difference.  Measured against the reference over
every case below: 0 ulp for values and gradients alike; the bound is ``SAMPLER_ULPS`` = 1 float32 ulp of the reference value (4 x 0, and
not below one ulp).
"""
import numpy as np
import pytest
import torch

import distance_field_cases as DC
import distance_field_ref as DR
import visual_hull_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLER_ULPS = 1.0
DYADIC = ((-1.5, 0.25, -0.75), 0.125)  # an origin and a voxel size whose cell centres float32 holds exactly


def _hull(occ, origin=(0.0, 0.0, 0.0), voxel=1.0):
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH

    N, Gz, Gy, Gx = occ.shape
    spec = engine.HullGridSpec(N, (Gx, Gy, Gz), origin, voxel)
    return VH.VisualHull(torch.from_numpy(np.ascontiguousarray(occ)).to(DEV), None, None, spec)


def _check_transform(occ, reference, combos=DC.COMBOS):
    hull = _hull(occ)
    for invert, border in combos:
        want = reference(invert, border)
        got = hull.distance_transform(inside=bool(invert), border=bool(border))
        assert got.dtype == torch.int32 and tuple(got.shape) == occ.shape
        bad = got.cpu().numpy().astype(np.int64) != want
        assert not bad.any(), (occ.shape, invert, border, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    again = hull.distance_transform(inside=bool(invert), border=bool(border))  # two calls: the same bits
    assert torch.equal(got, again)


@pytest.mark.parametrize("Gx", sorted({G[0] for G in DC.SHAPES}))
def test_grid_shapes(Gx):
    """Every pattern x (invert, border) on the grids with this Gx: 17 frames a call, the empty frame between two full ones."""
    for G in (g for g in DC.SHAPES if g[0] == Gx):
        _check_transform(DC.patterns(G), lambda invert, border, G=G: DC.reference(G, invert, border))


@pytest.mark.parametrize("G", DC.PATH_SHAPES, ids=lambda G: "x".join(map(str, G)))
def test_kernel_paths(G):
    """One grid per remaining path of the kernel, (2, 3, 513) and (128, 513, 1) among them: 513 = ``LDS_LINE + 1`` is one beyond the longest
    line the LDS path holds, so the global-memory search and its second buffer run.  Sparse features (and their complement for
    ``invert``), an empty frame in the middle."""
    assert DC.LDS_LINE == 512
    plain, inverted = DC.sparse_patterns(G)
    _check_transform(plain, lambda invert, border: DC.sparse_reference(G, invert, border), [(0, 0), (0, 1)])
    _check_transform(inverted, lambda invert, border: DC.sparse_reference(G, invert, border), [(1, 0), (1, 1)])


def test_beyond_2_31_voxels():
    """N = 33 600 frames of 40^3 = 2.15e9 voxels (2.2 GB of occupancy, 8.6 GB of distances): all empty but the first, the last and the two
    around element 2^31, which hold about 200 seeded features each and are compared with ``edt_brute``; every other frame is NONE."""
    from smilify_amd import _lib

    N, G = 33_600, 40
    vox = G ** 3
    assert N * vox > 2**31
    straddle = 2**31 // vox  # the frame that holds element 2^31
    frames = [0, straddle - 1, straddle, N - 1]
    assert straddle * vox < 2**31 < (straddle + 1) * vox
    rng = np.random.default_rng(2031)
    occ = torch.zeros(N, G, G, G, dtype=torch.uint8, device=DEV)
    small = (rng.random((4, G, G, G)) < 200.0 / vox).astype(np.uint8)
    assert all(100 < s.sum() < 300 for s in small)
    occ[frames] = torch.from_numpy(small).to(DEV)
    d2 = _hull_from_tensor(occ).distance_transform()
    want = DR.edt_brute(small)
    assert np.array_equal(d2[frames].cpu().numpy().astype(np.int64), want)
    d2[frames] = _lib.EDT_NONE
    assert bool((d2 == _lib.EDT_NONE).all())


def _hull_from_tensor(occ):
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH

    N, Gz, Gy, Gx = occ.shape
    return VH.VisualHull(occ, None, None, engine.HullGridSpec(N, (Gx, Gy, Gz), (0.0, 0.0, 0.0), 1.0))


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def _ulps(got, ref64):
    ref = ref64.astype(np.float32)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())


PER_FRAME = (np.array([[-0.31, 0.12, 0.05], [0.2, -0.4, 0.1], [0.013, -0.021, 0.017]]), np.array([0.11, 0.07, 0.093]))
SAMPLER_CASES = [  # (grid, (origin, voxel), point_dim)
    ((7, 6, 5), DYADIC, 3), ((7, 6, 5), PER_FRAME, 3), ((9, 1, 4), PER_FRAME, 3), ((1, 1, 1), DYADIC, 3), ((1, 5, 1), PER_FRAME, 3),
    ((12, 9, 1), DYADIC, 3), ((12, 9, 1), DYADIC, 2), ((12, 9, 1), PER_FRAME, 2), ((1, 1, 1), PER_FRAME, 2), ((66, 1, 1), DYADIC, 2),
]


@pytest.mark.parametrize("case", range(len(SAMPLER_CASES)))
def test_sampler_against_the_restatement(case):
    """Unsigned and signed fields of three frames, the middle one without a hull (NONE), shared (dyadic) and per-frame tables, grids with
    axes of one cell, P in {1, 63, 65}: cell centres, random positions, outside on every side / edge / corner, NaN and infinite points."""
    from smilify_amd import engine

    G, (origin, voxel), dim = SAMPLER_CASES[case]
    N = 3
    occ = DC.blob(G, N, seed=case)
    occ[1] = 0
    d_out, d_in = DR.edt_brute(occ, 0, 0), DR.edt_brute(occ, 1, 1)
    assert (d_out[1] == DR.NONE).all() and (d_in[1] < DR.NONE).all()
    spec = engine.HullGridSpec(N, G, origin, voxel)
    t_out, t_in = (torch.from_numpy(d.astype(np.int32)).to(DEV) for d in (d_out, d_in))
    worst = [0.0, 0.0]
    for P in (1, 63, 65):
        pts = DC.sample_points(G, origin, voxel, N, P, dim, seed=case)
        for signed in (False, True):
            value, grad = engine.field_sample(spec, t_out, t_in if signed else None, torch.from_numpy(pts).to(DEV))
            r_value, r_grad = DR.sample_ref(d_out, d_in if signed else None, origin, voxel, pts, dim)
            assert value.dtype == grad.dtype == torch.float32 and tuple(value.shape) == (N, P) and tuple(grad.shape) == (N, P, dim)
            value, grad = value.cpu().numpy(), grad.cpu().numpy()
            worst = [max(worst[0], _ulps(value, r_value)), max(worst[1], _ulps(grad, r_grad))]
            if signed and P == 65 and G == (7, 6, 5):
                assert (r_value < 0).any() and (r_value > 0).any()
            # a frame without a hull: nothing but the pull back to the box of cell centres; a non-finite point: nothing at all
            fin = np.isfinite(pts).all(-1)
            assert (value[~fin] == 0).all() and (grad[~fin] == 0).all()
            if P > 1:
                assert not fin.all()
            # at a cell centre of a dyadic grid the value is the cell's, exactly
            if origin is DYADIC[0] and dim == 3:
                u = (pts[:, 0::8].astype(np.float64) - np.array(origin)) / voxel - 0.5
                ok = np.isfinite(u).all(-1)
                assert np.array_equal(u[ok], np.rint(u[ok]))
                i, j, k = (np.where(ok, u[..., a], 0).astype(np.int64) for a in range(3))
                r = np.sqrt(d_out.astype(np.float64)) - (np.sqrt(d_in.astype(np.float64)) if signed else 0.0)
                r = np.where(d_out == DR.NONE, 0.0, r)
                cell = (voxel * r[np.arange(N)[:, None], k, j, i]).astype(np.float32)
                assert np.array_equal(value[:, 0::8][ok], cell[ok])
            no_grad, none = engine.field_sample(spec, t_out, t_in if signed else None, torch.from_numpy(pts).to(DEV), want_grad=False)
            assert none is None and np.array_equal(no_grad.cpu().numpy(), value)
    print(f"sampler case {case} {G} dim {dim}: max error {worst[0]:.3g} ulp (value), {worst[1]:.3g} ulp (gradient)")
    assert max(worst) <= SAMPLER_ULPS


def test_sampler_rejects_bad_arguments():
    from smilify_amd import _lib, engine

    spec = engine.HullGridSpec(1, (4, 4, 2), (0.0, 0.0, 0.0), 0.5)
    d2 = torch.zeros(1, 2, 4, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.SmilError, match="needs Gz=1"):
        engine.field_sample(spec, d2, None, torch.zeros(1, 3, 2, device=DEV))
    with pytest.raises(ValueError):
        engine.field_sample(spec, d2.long(), None, torch.zeros(1, 3, 3, device=DEV))
    with pytest.raises(_lib.SmilError, match="positive and finite"):
        engine.field_sample(engine.HullGridSpec(1, (4, 4, 2), (0.0, 0.0, 0.0), 0.0), d2, None, torch.zeros(1, 3, 3, device=DEV))
    value, grad = engine.field_sample(spec, d2, None, torch.zeros(1, 0, 3, device=DEV))
    assert tuple(value.shape) == (1, 0) and tuple(grad.shape) == (1, 0, 3)


def test_autograd_and_containment_loss():
    """``sample(points).sum().backward()`` leaves the reference's gradient; a weighted upstream gradient scales it; ``containment_loss`` is
    the (weighted) mean of the squares."""
    G, (origin, voxel) = (7, 6, 5), PER_FRAME
    occ = DC.blob(G, 3, seed=4)
    hull = _hull(occ, origin, voxel)
    for signed in (False, True):
        field = hull.distance_field(signed=signed)
        assert field.signed == signed and field.d2_out.dtype == torch.int32 and (field.d2_in is not None) == signed
        d_out, d_in = DR.edt_brute(occ, 0, 0), DR.edt_brute(occ, 1, 1)
        assert np.array_equal(field.d2_out.cpu().numpy(), d_out) and (not signed or np.array_equal(field.d2_in.cpu().numpy(), d_in))
        pts = DC.sample_points(G, origin, voxel, 3, 65, 3, seed=9)
        r_value, r_grad = DR.sample_ref(d_out, d_in if signed else None, origin, voxel, pts, 3)
        x = torch.from_numpy(pts).to(DEV).requires_grad_(True)
        value = field.sample(x)
        value.sum().backward()
        assert _ulps(value.detach().cpu().numpy(), r_value) <= SAMPLER_ULPS and _ulps(x.grad.cpu().numpy(), r_grad) <= SAMPLER_ULPS
        w = torch.linspace(0.0, 2.0, 3 * 65, device=DEV).reshape(3, 65)
        x2 = torch.from_numpy(pts).to(DEV).requires_grad_(True)
        (field.sample(x2) * w).sum().backward()
        assert torch.equal(x2.grad, w[..., None] * x.grad)
        assert not field.sample(x.detach()).requires_grad
        s = value.detach().double()
        assert abs(float(field.containment_loss(x.detach())) - float((s * s).mean())) <= 1e-6 * float((s * s).mean())
        want = float((w.double() * s * s).sum() / w.double().sum())
        assert abs(float(field.containment_loss(x.detach(), w)) - want) <= 1e-6 * want


def test_descent_into_a_carved_hull():
    """The ``ellipsoid32`` hull (8 views); 64 points 0.3 outside the ellipsoid along its rays from the centre, inside the grid; 200 plain
    gradient steps on ``containment_loss`` with the step 8 (every point moves a quarter of its distance per step).  Every point ends
    inside every outline (``query_points``: fg == seen == 8) or within one voxel of an occupied voxel's centre, which is such a point.
    The loss must fall from step to step.  The field is piecewise trilinear, so a step that crosses a cell face could overshoot; measured,
    none does: every one of the 200 steps lowers the loss (0.0938 -> 3.2e-9; the largest change between two steps is -4.0e-10 of the
    first loss).  The tolerance for a rise is 1e-6 of the first loss: the float32 rounding of a mean of 64 squares near convergence."""
    from smilify_amd import visual_hull as VH

    c = VC.get("ellipsoid32")
    masks = torch.from_numpy(c.masks).to(DEV)
    cams = {k: torch.from_numpy(v) for k, v in c.cams.items()}
    hull = VH.carve(masks, cams, image_size=c.S, origin=c.origin, voxel_size=c.voxel_size, grid=c.grid, min_views=c.min_views)
    field = hull.distance_field()
    centre, radii = c.ellipsoids[0]
    rng = np.random.default_rng(5)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    start = centre + d * (1.0 / np.sqrt(((d / radii) ** 2).sum(1)) + 0.3)[:, None]
    lo, hi = c.origin[0] + 0.5 * c.voxel_size[0], c.origin[0] + (np.array(c.grid) - 0.5) * c.voxel_size[0]
    start = start[((start > lo) & (start < hi)).all(1)][:64]
    assert start.shape == (64, 3)
    x = torch.from_numpy(start.astype(np.float32)).to(DEV)[None].requires_grad_(True)
    fg, seen = VH.query_points(x.detach(), masks, cams, image_size=c.S)
    assert not ((fg == c.views) & (seen == c.views)).any()  # every point starts outside some outline
    losses = []
    for _ in range(200):
        loss = field.containment_loss(x)
        (g,) = torch.autograd.grad(loss, x)
        losses.append(loss.detach())
        with torch.no_grad():
            x -= 8.0 * g
    losses = torch.stack(losses + [field.containment_loss(x).detach()]).cpu().numpy().astype(np.float64)
    rise = float(np.diff(losses).max() / losses[0])
    print(f"descent: loss {losses[0]:.4g} -> {losses[-1]:.4g}, largest rise between steps {rise:.3g} of the first loss")
    assert rise <= 1e-6 and losses[-1] < 1e-6 * losses[0]
    fg, seen = VH.query_points(x.detach(), masks, cams, image_size=c.S)
    inside = ((fg == c.views) & (seen == c.views))[0].cpu().numpy()
    occ = hull.occupancy[0].cpu().numpy()
    k, j, i = np.nonzero(occ)
    centres = c.origin[0] + (np.stack([i, j, k], 1) + 0.5) * c.voxel_size[0]
    end = x.detach()[0].cpu().numpy().astype(np.float64)
    near = np.sqrt(((end[:, None, :] - centres[None]) ** 2).sum(-1).min(1))
    print(f"descent: {int(inside.sum())} of 64 inside every outline, farthest from an occupied centre {near.max() / c.voxel_size[0]:.3f} voxels")
    assert (inside | (near <= c.voxel_size[0])).all()


# ---- the 2-D form -----------------------------------------------------------------------------------------------------------
def _masks_2d(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fg = np.zeros((2, 3, H, W), bool)
    for n in range(2):
        for v in range(3):
            cy, cx, r = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.1, 0.3) * min(H, W) + 0.6
            fg[n, v] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    fg[1, 1] = False  # an image without foreground
    return fg


@pytest.mark.parametrize("H,W", [(48, 80), (1, 1)])
def test_mask_distance_transform(H, W):
    """uint8, bool and float32 masks (a threshold, a NaN pixel that counts as background), (N,Nv,H,W) and (N,H,W), outside and inside."""
    from smilify_amd import imageprep

    fg = _masks_2d(H, W, seed=H)
    if H == 1:
        fg[0, 0] = True
    f32 = np.where(fg, 0.8, 0.3).astype(np.float32)
    nan_at = tuple(np.argwhere(fg)[len(np.argwhere(fg)) // 2])
    f32[nan_at] = np.nan
    fg_nan = fg.copy()
    fg_nan[nan_at] = False
    for masks, thr, truth in (((fg * 200).astype(np.uint8), 0.0, fg), (fg, 0.0, fg), (f32, 0.5, fg_nan), ((fg * 3).astype(np.uint8), 3.0, fg & False)):
        for inside in (False, True):
            got = imageprep.mask_distance_transform(torch.from_numpy(masks).to(DEV), threshold=thr, inside=inside)
            want = DR.edt_brute(truth.reshape(-1, 1, H, W), inside).reshape(truth.shape)
            assert got.dtype == torch.int32 and tuple(got.shape) == masks.shape
            assert np.array_equal(got.cpu().numpy(), want), (masks.dtype, inside)
    got = imageprep.mask_distance_transform(torch.from_numpy(fg[:, 0]).to(DEV))  # (N,H,W)
    assert tuple(got.shape) == (2, H, W) and np.array_equal(got.cpu().numpy(), DR.edt_brute(fg[:, 0][:, None])[:, 0])
    assert bool((imageprep.mask_distance_transform(torch.from_numpy(fg).to(DEV))[1, 1] == DR.NONE).all())


def test_sample_mask_distance():
    """At pixel centres (r + 0.5, c + 0.5) the value is sqrt(d2) of the pixel, exactly; at random points (some outside the image) value and
    gradient are the restatement's with point_dim = 2, origin 0 and voxel 1; (N,Nv,H,W) and (N,H,W) forms."""
    from smilify_amd import imageprep

    H, W, P = 48, 80, 65
    fg = _masks_2d(H, W, seed=3)
    d2 = imageprep.mask_distance_transform(torch.from_numpy(fg).to(DEV))
    d2_np = d2.cpu().numpy()
    rng = np.random.default_rng(8)
    rc = np.stack([rng.integers(0, H, (2, 3, P)), rng.integers(0, W, (2, 3, P))], -1)
    centres = torch.from_numpy((rc + 0.5).astype(np.float32)).to(DEV)
    got = imageprep.sample_mask_distance(d2, centres)
    n, v = np.arange(2)[:, None, None], np.arange(3)[None, :, None]
    cell = d2_np[n, v, rc[..., 0], rc[..., 1]]
    want = np.where(cell == DR.NONE, 0.0, np.sqrt(cell.astype(np.float64))).astype(np.float32)
    assert tuple(got.shape) == (2, 3, P) and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    pts = rng.uniform(-4.0, 1.0, (2, 3, P, 2)) + rng.uniform(0.0, 1.0, (2, 3, P, 2)) * np.array([H + 3.0, W + 3.0])
    pts = pts.astype(np.float32)
    pts[0, 0, 0, 1] = np.nan
    x = torch.from_numpy(pts).to(DEV).requires_grad_(True)
    value = imageprep.sample_mask_distance(d2, x)
    value.sum().backward()
    r_value, r_grad = DR.sample_ref(d2_np.reshape(6, 1, H, W), None, np.zeros((1, 3)), np.ones(1), pts.reshape(6, P, 2), 2)
    assert _ulps(value.detach().cpu().numpy().reshape(6, P), r_value) <= SAMPLER_ULPS and _ulps(x.grad.cpu().numpy().reshape(6, P, 2), r_grad) <= SAMPLER_ULPS
    assert (r_value > 0).mean() > 0.5 and (np.abs(r_grad).sum(-1) > 0).mean() > 0.5
    flat = imageprep.sample_mask_distance(d2[:, 0].contiguous(), x.detach()[:, 0].contiguous())  # (N,H,W) with (N,P,2)
    assert torch.equal(flat, value.detach()[:, 0])
    with pytest.raises(ValueError):
        imageprep.sample_mask_distance(d2, x.detach()[:, 0])


def test_projected_joints_on_rendered_masks(tables):
    """The composition a fitter would write: the synthetic model's joints through ``keypoint_losses.project_joints_to_views``, scaled to
    pixels, sampled on the distance transform of masks ``Renderer`` rendered with the true cameras.  With the cameras' T displaced, a
    backward pass leaves finite, non-zero gradients on T, and one Adam step on T alone lowers the loss."""
    from smilify_amd import engine, imageprep, keypoint_losses, synthetic
    from smilify_amd.p3d_renderer import Renderer

    t = tables("synthetic")
    S, views = 64, 3
    dm = engine.DeviceModel(t, DEV)
    pose, trans = synthetic.random_pose(1, t.J, torch.Generator().manual_seed(5))
    out = engine.lbs_forward(dm, torch.zeros(t.nB, device=DEV), pose.to(DEV).contiguous(), trans=trans.to(DEV).contiguous(), shared_beta=True,
                             trans_after_joints=True)
    R, T = synthetic.camera_ring(views, 2.7)
    fov = torch.full((1,), 60.0)
    r = Renderer(S, DEV, views=views)
    r.set_camera_parameters(R, T, fov)
    faces = torch.from_numpy(t.faces.astype(np.int64)).to(DEV)[None]
    masks = (r.render_fragments(out["verts"], faces, want=("pix_to_face",)).pix_to_face >= 0).reshape(1, views, S, S)
    assert masks.any(dim=-1).any(dim=-1).all()
    d2 = imageprep.mask_distance_transform(masks)
    joints = out["joints"].detach().reshape(1, t.J, 3)
    Rv, fv = R.to(DEV).reshape(1, views, 3, 3), fov.to(DEV).expand(1, views).contiguous()

    def loss_of(Tv):
        yx = keypoint_losses.project_joints_to_views(joints, Rv, Tv, fv, S) * (S + 1e-8)
        return (imageprep.sample_mask_distance(d2, yx) ** 2).mean()

    true_T = T.to(DEV).reshape(1, views, 3)
    at_truth = float(loss_of(true_T))
    Tv = (true_T + torch.tensor([0.35, -0.25, 0.1], device=DEV)).clone().requires_grad_(True)
    loss = loss_of(Tv)
    loss.backward()
    assert torch.isfinite(Tv.grad).all() and (Tv.grad.abs().amax(dim=-1) > 0).all()
    assert float(loss.detach()) > at_truth and float(loss.detach()) > 0.0  # the displaced joints lie off the silhouettes
    opt = torch.optim.Adam([Tv], lr=0.02)
    opt.step()
    after = float(loss_of(Tv.detach()))
    print(f"projected joints: loss {at_truth:.4g} at the true cameras, {float(loss.detach()):.4g} displaced, {after:.4g} after one Adam step on T")
    assert after < float(loss.detach())
