"""GPU tests of ``smilify_amd.imageprep`` (``pytest -m gpu``): ``crop_to_silhouette`` against what the reference returned
(tests/golden/imageprep_ref.npz), the invariants that tie ``prepare_targets`` to ``undistort_images`` and to the lens-less warp, the
half-pixel convention of the fused route against the renderer, and a ``SMALFitter`` built from ``prepare_targets`` output.

Tolerances are those of tests/test_gpu_imageprep_kernels.py (its docstring derives them): nearest results exact, bilinear results
``|d| <= 2e-6 M`` with M the largest tap magnitude; joints 1e-12 px (float64 on both sides, two roundings of numbers below 100)."""
import numpy as np
import pytest
import torch

import imageprep_cases as CASES
import test_gpu_cameras as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BILINEAR_RTOL = 2e-6
SIZES = (5, 8, 17)

t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731


@pytest.mark.parametrize("g", ["a", "b"])
def test_crop_to_silhouette_reference_fixture(g, golden):
    """One image at a time through the reference's signature, and all three as a batch (arrays and tensors): the mask equal, the RGB
    image to the bilinear bound (M = 1: values in [0, 1], padding 1), the joints to 1e-12."""
    from smilify_amd import imageprep as ip

    fx = golden("imageprep_ref")
    sil, rgb, joints = fx[f"{g}_sil"], fx[f"{g}_rgb"], fx[f"{g}_joints"]
    bounds, windows = ip.silhouette_windows(sil)
    assert bounds.dtype == np.int32 and np.array_equal(bounds, fx[f"{g}_bounds"])
    assert windows.dtype == np.float64 and np.array_equal(windows, fx[f"{g}_windows"])
    worst = 0.0
    for S in SIZES:
        want = [fx[f"{g}_S{S}_{k}"] for k in ("sil", "rgb", "joints")]
        for n in range(3):
            s, r, j = ip.crop_to_silhouette(sil[n], rgb[n], joints[n], S)
            assert isinstance(s, np.ndarray) and s.shape == (S, S) and r.shape == (S, S, 3) and j.shape == joints[n].shape
            assert np.array_equal(s, want[0][n]), (g, S, n)
            worst = max(worst, float(np.abs(r.astype(np.float64) - want[1][n]).max()))
            np.testing.assert_allclose(j, want[2][n], rtol=0, atol=1e-12)
        for conv in (lambda a: a, t):
            s, r, j = ip.crop_to_silhouette(conv(sil), conv(rgb), conv(joints), S)
            if conv is t:
                assert s.device.type == "cuda" and r.device.type == "cuda"
                s, r, j = s.cpu().numpy(), r.cpu().numpy(), j.cpu().numpy()
            assert np.array_equal(s, want[0])
            worst = max(worst, float(np.abs(r.astype(np.float64) - want[1]).max()))
            np.testing.assert_allclose(j, want[2], rtol=0, atol=1e-12)
    print(f"crop_to_silhouette {g}: RGB max |d| {worst:.3e} (bound {BILINEAR_RTOL:.1e})")
    assert worst <= BILINEAR_RTOL
    for bad, match in ((fx[f"{g}_onepx_sil"], "side 0"), (np.zeros_like(sil[0]), "no foreground")):  # where the reference fails too
        with pytest.raises(ValueError, match=match):
            ip.crop_to_silhouette(bad, rgb[0], joints[0], 8)
    with pytest.raises(ValueError, match=r"image\(s\) \[1\]"):
        ip.silhouette_windows(np.stack([sil[0], np.zeros_like(sil[0]), sil[2]]))


def test_resize_images_is_the_crop_of_the_whole_image(golden):
    """resize_images is crop_to_silhouette's pair of resizes with the image as the square: against the restatement's resize."""
    import imageprep_ref as IR
    from smilify_amd import imageprep as ip

    fx = golden("imageprep_ref")
    rgb, sil = fx["a_rgb"], fx["a_sil"]
    for size in ((5, 8), (17, 30)):
        want = np.stack([IR.resize(im, (size[1], size[0]), "linear") for im in rgb])
        got = ip.resize_images(rgb, size, "linear")
        assert got.shape == (3,) + size + (3,) and np.abs(got.astype(np.float64) - want).max() <= BILINEAR_RTOL
        want = np.stack([IR.resize(im, (size[1], size[0]), "nearest") for im in sil])
        assert np.array_equal(ip.resize_images(sil, size, "nearest"), want)
        assert np.array_equal(ip.resize_images(t(sil[0]), size, "nearest").cpu().numpy(), want[0])


def _frames(rng, N, H, W):
    frames = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    masks = (rng.uniform(size=(N, H, W)) < 0.4).astype(np.uint8)
    return frames, masks


def test_prepare_targets_is_undistortion_then_slicing():
    """Integer x0, y0 and side == S: the fused route equals undistort_images followed by array slicing, with the border (1 for frames,
    0 for masks) where the slice leaves the image - equal for the masks, to the bilinear bound (M = 255, scaled by 1/255) for frames.
    The lens is a pincushion (k1 > 0): what lies outside the undistorted image then maps outside the frame, which is what the
    invariant is about - the fused route has no notion of the undistorted image's extent and, under a barrel lens, shows the frame's
    content there instead of a border."""
    from smilify_amd import engine, imageprep as ip

    rng = np.random.default_rng(5)
    N, H, W, S = 3, 13, 21, 8
    frames, masks = _frames(rng, N, H, W)
    K, dist = CASES.K_A, np.array([0.21, 0.05, 0.004, -0.006, 0.01])
    windows = np.array([[4.0, 2.0, S], [-3.0, 9.0, S], [16.0, -5.0, S]])
    joints = rng.uniform(0.0, 13.0, (N, 6, 2))
    rgb, sil, j = ip.prepare_targets(frames, masks, K, dist, windows, S, joints_yx=joints)
    assert rgb.shape == (N, 3, S, S) and sil.shape == (N, 1, S, S) and rgb.dtype == sil.dtype == np.float32
    np.testing.assert_allclose(j, joints - windows[:, None, [1, 0]], rtol=0, atol=1e-12)

    und = ip.undistort_images(frames, K, dist)                                 # (N,H,W,3) float32 of 0 .. 255, border 0
    assert und.shape == frames.shape and und.dtype == np.float32 and not np.array_equal(und, frames)
    und_u8 = ip.undistort_images(frames, K, dist, dtype=np.uint8)             # the rounded float result (not OpenCV's fixed-point remap)
    assert und_u8.dtype == np.uint8 and np.array_equal(und_u8, np.rint(np.clip(und, 0.0, 255.0)).astype(np.uint8))
    one = ip.undistort_images(frames[1], K, dist, new_K=K)                      # one image, as cv2.undistort takes it
    assert one.shape == frames[1].shape and np.array_equal(one, und[1])
    lens = [t(a[None]) for a in (K, K, dist)]
    und_mask = engine.warp_images(t(masks), (H, W), t(np.array([[1.0, 0.0, 1.0, 0.0]])), interpolation="nearest", K=lens[0], K_new=lens[1],
                                  dist=lens[2]).cpu().numpy()
    inside = engine.warp_images(t(np.ones((N, H, W), np.float32)), (H, W), t(np.array([[1.0, 0.0, 1.0, 0.0]])), K=lens[0], K_new=lens[1],
                                dist=lens[2]).cpu().numpy()                     # the bilinear weight of what lies inside the frame
    worst = 0.0
    for n, (x0, y0, _) in enumerate(windows.astype(int)):
        want_rgb, want_sil = np.ones((S, S, 3)), np.zeros((S, S), np.float32)
        ys, xs = [i for i in range(S) if 0 <= y0 + i < H], [k for k in range(S) if 0 <= x0 + k < W]
        yy, xx = np.ix_(ys, xs)
        # undistort_images pads with 0 where the fused route pads with 1: the missing weight is 1 - inside
        want_rgb[yy, xx] = und[n][y0 + yy, x0 + xx].astype(np.float64) / 255.0 + (1.0 - inside[n][y0 + yy, x0 + xx].astype(np.float64))[..., None]
        want_sil[yy, xx] = und_mask[n][y0 + yy, x0 + xx]
        assert np.array_equal(sil[n, 0], want_sil), n
        worst = max(worst, float(np.abs(rgb[n].transpose(1, 2, 0) - want_rgb).max()))
        assert len(ys) < S or len(xs) < S or n == 0
    print(f"prepare_targets vs undistort + slice: frames max |d| {worst:.3e}")
    assert worst <= BILINEAR_RTOL


def test_zero_distortion_invariants():
    """Zero dist: undistort_images hands back its input object, and prepare_targets equals the lens-less warp bit for bit.

    That the lens is skipped is one half; that the lens-less map is the documented one is the other, and it is checked against
    expectations written here from the convention and not from the product's expression of it: output pixel j is centred at
    x0 + (j + 0.5) side / S of the source's pixel GRID (pixel k covers [k, k + 1)), so the nearest sample is the pixel that contains
    that point, floor(x0 + (j + 0.5) side / S), and the bilinear sample is the restatement's at the coordinate minus one half.  The
    windows (side / S = 19 / 34 and 21 / 17, x0 and y0 multiples of 0.1) keep every such point at least 0.4 / 68 px from a pixel edge,
    so the last bits of the two expressions cannot change a tap."""
    import imageprep_ref as IR
    from smilify_amd import engine, imageprep as ip

    rng = np.random.default_rng(6)
    frames, masks = _frames(rng, 2, 16, 16)
    tf = t(frames)
    for d in (None, np.zeros(5), np.zeros((2, 5)), torch.zeros(5)):
        assert ip.undistort_images(frames, CASES.K_B, d) is frames
        assert ip.undistort_images(tf, CASES.K_B, d) is tf
    win, S = np.array([[2.3, -1.7, 9.5], [5.0, 4.0, 21.0]]), 17
    step = win[:, 2] / S
    c = ip.FUSED_CENTRE
    affine = t(np.stack([step, win[:, 0] + c * (step - 1.0), step, win[:, 1] + c * (step - 1.0)], axis=1))
    want_rgb = engine.warp_images(tf, S, affine, planar=True, border=t(np.full((1, 3), 255.0, np.float32)), scale=1.0 / 255.0)
    want_sil = engine.warp_images(t(masks), S, affine, interpolation="nearest", planar=True)
    for d in (None, np.zeros(5)):
        rgb, sil, j = ip.prepare_targets(tf, t(masks), CASES.K_B, d, win, S)
        assert j is None and rgb.device.type == "cuda" and torch.equal(rgb, want_rgb) and torch.equal(sil, want_sil)
    assert 0.0 < float(want_sil.mean()) < 1.0 and float(want_rgb.max()) == 1.0

    containing = np.zeros((2, 1, S, S), np.float32)  # the source pixel that contains the output pixel's centre; 0 outside the image
    for n, (x0, y0, side) in enumerate(win):
        for i in range(S):
            for k in range(S):
                x, y = int(np.floor(x0 + (k + 0.5) * side / S)), int(np.floor(y0 + (i + 0.5) * side / S))
                if 0 <= x < 16 and 0 <= y < 16:
                    containing[n, 0, i, k] = masks[n, y, x]
    assert np.array_equal(sil.cpu().numpy(), containing)
    centres = np.stack([step, win[:, 0] + 0.5 * step - 0.5, step, win[:, 1] + 0.5 * step - 0.5], axis=1)
    restated = IR.warp(frames, S, centres, border=np.full((1, 3), 255.0), scale=1.0 / 255.0, planar=True)
    err = float(np.abs(rgb.cpu().numpy().astype(np.float64) - restated).max())
    print(f"prepare_targets without a lens vs the restatement at the pixel centres: frames max |d| {err:.3e}")
    assert err <= BILINEAR_RTOL  # (M = 255, after the scale of 1 / 255)


def _stick_scene(tables):
    from smilify_amd.smal_torch import SMAL

    tb = tables("stick")
    smal = SMAL(DEV, tables=tb)
    theta = 0.2 * torch.randn(1, tb.J, 3, generator=torch.Generator().manual_seed(2))
    verts, _, _, _ = smal(torch.zeros(1, tb.nB, device=DEV), theta.to(DEV))
    return smal, verts.detach()


def _coverage(smal, verts, cal, S, window=None):
    """The hard coverage mask (S,S) uint8 of the mesh through opencv_to_pinhole_camera(R, t, K, S, window)."""
    from smilify_amd import cameras
    from smilify_amd.p3d_renderer import Renderer

    R, T, fov, aspect, pp = cameras.opencv_to_pinhole_camera(*cal, S, window=window)
    rend = Renderer(S, DEV)
    rend.set_camera_parameters(torch.tensor(R)[None], torch.tensor(T)[None], torch.tensor([fov], dtype=torch.float32),
                               aspect_ratio=torch.tensor([aspect], dtype=torch.float32), principal_point=torch.tensor(pp, dtype=torch.float32)[None])
    frag = rend.render_fragments(verts, smal.faces, want=("pix_to_face",))
    return (frag.pix_to_face[0] >= 0).to(torch.uint8)


def _window_on_the_silhouette(mask64, side):
    """Integer (x0, y0) of a window of `side` whose left border runs through the silhouette's median foreground pixel (the model is a
    stick figure: thin limbs), so that the window cuts it."""
    ys, xs = np.nonzero(mask64)
    k = np.argsort(xs, kind="stable")[len(xs) // 2]
    x0, y0 = int(xs[k]), int(ys[k]) - side // 2
    return min(max(x0, 0), 64 - side), min(max(y0, 0), 64 - side)


def test_fused_convention_against_the_renderer(tables):
    """The renderer is the yardstick.  STICK, hard coverage masks: the 64 x 64 render through opencv_to_pinhole_camera(R, t, K, 64) and
    the 32 x 32 render through the same calibration with window = (x0, y0, 32), integer x0, y0, the silhouette cut by the window.
    prepare_targets (masks, nearest, zero dist) of the 64-render with that window must differ from the direct 32-render in fewer than
    one tenth as many pixels as the best of the four windows shifted by +-1 px in x or y."""
    from smilify_amd import imageprep as ip

    smal, verts = _stick_scene(tables)
    cal = tc._calibrations(1, 64, seed=4)[0]
    m64 = _coverage(smal, verts, cal, 64)
    x0, y0 = _window_on_the_silhouette(m64.cpu().numpy(), 32)
    direct = _coverage(smal, verts, cal, 32, window=(x0, y0, 32))
    cut, whole = direct.cpu().numpy(), m64.cpu().numpy()
    # cut by the window: foreground on its left border, inside it and outside it
    assert cut[:, 0].any() and 20 < cut.sum() < whole.sum() - 20, (x0, y0, int(cut.sum()), int(whole.sum()))
    frames = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV)

    def differing(window):
        _, sil, _ = ip.prepare_targets(frames, m64[None], cal[2], np.zeros(5), np.asarray(window, np.float64), 32)
        return int((sil[0, 0] != direct).sum())

    own = differing((x0, y0, 32))
    shifted = [differing((x0 + dx, y0 + dy, 32)) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))]
    print(f"window ({x0}, {y0}, 32): {own} pixels differ from the direct render; shifted by +x, -x, +y, -y: {shifted}")
    assert 10 * own < min(shifted), (own, shifted)


def test_fused_convention_against_the_renderer_when_resizing(tables):
    """side != S is where the pixel-centre question shows (for side == S every answer agrees): the 64-render magnified 2 x (a window of
    side 16 to S = 32) against the direct 32-render of that window.  With the renderer's pixel centres at j + 0.5 the nearest source
    pixel of output pixel j is the one that CONTAINS its centre, floor(x0 + (j + 0.5) / 2): prepare_targets must beat the same window
    moved by half a source pixel in +-x and +-y (every second output pixel then reads the neighbouring source pixel) and moved by
    (+0.25, +0.25), which is the pixel-index reading x0 + j side / S of cameras.crop_points_yx (every second pixel again: j / 2 + 0.5
    rounds up for odd j).  Strictly fewer differing pixels.  (A move by -0.25 changes no tap at this magnification: it is no
    alternative.)"""
    from smilify_amd import imageprep as ip

    smal, verts = _stick_scene(tables)
    cal = tc._calibrations(1, 64, seed=4)[0]
    m64 = _coverage(smal, verts, cal, 64)
    x0, y0 = _window_on_the_silhouette(m64.cpu().numpy(), 16)
    direct = _coverage(smal, verts, cal, 32, window=(x0, y0, 16))
    assert direct[:, 0].any() and 20 < int(direct.sum()) < 32 * 32 - 20, (x0, y0, int(direct.sum()))
    frames = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV)

    def differing(window):
        _, sil, _ = ip.prepare_targets(frames, m64[None], cal[2], None, np.asarray(window, np.float64), 32)
        return int((sil[0, 0] != direct).sum())

    own = differing((x0, y0, 16))
    moved = {d: differing((x0 + d[0], y0 + d[1], 16)) for d in ((0.5, 0), (-0.5, 0), (0, 0.5), (0, -0.5), (0.25, 0.25))}
    print(f"window ({x0}, {y0}, 16) to 32: {own} pixels differ from the direct render; moved: {moved}")
    assert own < min(moved.values()), (own, moved)


def test_fitter_accepts_prepared_targets(tables):
    """End to end: three frames of a synthetic scene at 64 x 64, prepared to S = 32 with the whole frame as the window (the camera
    stays the scene's: crop_intrinsics only scales it), make a SMALFitter whose fit step returns finite losses."""
    from smilify_amd import imageprep as ip, synthetic
    from smilify_amd.fitter import SMALFitter

    tb = tables("stick")
    scene = synthetic.make_problem(tb, 3, 1, 64, DEV, seed=21, window=3)
    masks = scene.sil_imgs[:, 0]
    frames = (masks[..., None] * torch.tensor([200, 120, 40], dtype=torch.uint8, device=DEV)).contiguous()
    rgb, sil, joints = ip.prepare_targets(frames, masks, np.array([[55.0, 0, 32], [0, 55.0, 32], [0, 0, 1]]), None, (0.0, 0.0, 64.0), 32,
                                          joints_yx=scene.target_joints)
    assert rgb.shape == (3, 3, 32, 32) and sil.shape == (3, 1, 32, 32) and joints.shape == scene.target_joints.shape
    assert torch.equal(joints, scene.target_joints * 0.5)
    assert 0.0 < float(sil.mean()) < 1.0 and set(sil.unique().tolist()) == {0.0, 1.0}
    fitter = SMALFitter(DEV, (rgb, sil, joints, scene.target_visibility), 3, -1, False, tables=tb, config=scene.config, views=1)
    fitter.set_cameras(scene.renderer.cameras.R, scene.renderer.cameras.T)
    assert fitter.image_size == 32 and fitter.num_images == 3
    fitter.begin_stage(synthetic.STAGE1_LR)
    objs = fitter.fit_step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL, window=3)
    torch.cuda.synchronize()
    assert torch.isfinite(objs).all() and float(objs[:9].sum()) > 0.0, objs
