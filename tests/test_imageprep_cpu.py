"""CPU-side checks of the target image preparation: the float64 restatement (tests/imageprep_ref.py) against what the reference's
crop_to_silhouette returned (tests/golden/imageprep_ref.npz, written by tests/golden/make_imageprep_fixture.py), the window formula of
the product, the premises of the GPU warp cases, and every argument check of the wrappers and of the C entry points - none of which
touches a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import imageprep_cases as CASES
import imageprep_ref as IR

GROUPS, SIZES = ("a", "b"), (5, 8, 17)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("imageprep_ref")


@pytest.mark.parametrize("g", GROUPS)
def test_restatement_reproduces_the_reference(fx, g):
    """The restated crop (bounds, window, ONE warp per image) equals what the reference made with its padding, slicing and resize."""
    sil, rgb, joints = fx[f"{g}_sil"], fx[f"{g}_rgb"], fx[f"{g}_joints"]
    for S in SIZES:
        for n in range(3):
            s, r, j = IR.crop_to_silhouette(sil[n], rgb[n], joints[n], S)
            assert np.array_equal(s, fx[f"{g}_S{S}_sil"][n]), (g, S, n)
            assert np.array_equal(r, fx[f"{g}_S{S}_rgb"][n]), (g, S, n)
            np.testing.assert_allclose(j, fx[f"{g}_S{S}_joints"][n], rtol=0, atol=1e-12)
            assert s.min() == 0.0 and s.max() > 0.0  # (every crop shows foreground and background)


@pytest.mark.parametrize("g", GROUPS)
def test_window_formula_matches_the_reference(fx, g):
    from smilify_amd import imageprep

    assert np.array_equal(IR.bounds(fx[f"{g}_sil"]), fx[f"{g}_bounds"])
    win = imageprep.windows_from_bounds(fx[f"{g}_bounds"])
    assert win.dtype == np.float64 and np.array_equal(win, fx[f"{g}_windows"])
    # the one-pixel mask: a square of side 0, on which the reference fails
    assert bool(fx[f"{g}_onepx_reference_raises"])
    one = imageprep.windows_from_bounds(fx[f"{g}_onepx_bounds"])[0]
    assert np.array_equal(one, fx[f"{g}_onepx_window"]) and one[2] == 0.0
    # the reference's joints are those of the window: (joints - (y0, x0)) * (S / side)
    for S in SIZES:
        for n in range(3):
            x0, y0, side = win[n]
            np.testing.assert_allclose(fx[f"{g}_S{S}_joints"][n], (fx[f"{g}_joints"][n] - [y0, x0]) * (S / side), rtol=0, atol=1e-12)


def test_fixture_covers_what_it_claims(fx):
    H, W = fx["a_sil"].shape[1:]
    assert (H, W) == (13, 21) and fx["b_sil"].shape[1:] == (16, 16)
    b = fx["a_bounds"][0]
    assert tuple(b[:4]) == (0, H - 1, 0, W - 1)          # touches all four edges ...
    assert fx["a_windows"][0][1] < 0                      # ... and its square reaches into the padding
    for g, width in (("a", 21), ("b", 16)):
        assert fx[f"{g}_windows"][2][0] + fx[f"{g}_windows"][2][2] > width  # the corner blob's square overhangs the right edge
    assert all(int(s) % 2 == 0 for s in fx["a_windows"][:, 2])
    sides = np.concatenate([fx["a_windows"][:, 2], fx["b_windows"][:, 2]])
    assert (sides > 5).any() and (sides < 17).any()      # both up- and down-scaling occur


def test_empty_mask_raises_naming_the_images():
    from smilify_amd import imageprep

    b = np.array([[0, 3, 1, 4, 7], [13, -1, 21, -1, 0], [2, 2, 2, 2, 1], [13, -1, 21, -1, 0]], np.int32)
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        imageprep.windows_from_bounds(b)


def test_nearest_samples_with_a_lens_keep_clear_of_rounding_boundaries():
    """The premise of the exact nearest comparisons on the GPU: with a lens the coordinate is a float64 polynomial, and a sample within
    rounding distance of k + 0.5 could fall either way.  None does - no pixel is left out of any comparison.  And the product takes
    each of these lenses as one: none is "all close to 0", which its wrappers skip."""
    from smilify_amd import imageprep

    lens = CASES.lens_cases()
    assert len(lens) >= 5
    for name, case in lens.items():
        assert CASES.nearest_margin(case) > 1e-9, name
        K, K_new, dist = case["lens"]
        tables = imageprep._lens(name, K, dist, K_new, len(dist), torch.device("cpu"))
        assert tables is not None and np.array_equal(tables[2].numpy(), dist), name


def test_strong_lens_leaves_the_image_and_overflows():
    """The a_strong case does what its name says, and the product's wrappers hand such coefficients on as they are (they refuse
    nothing for being large: what the coordinates then do is the kernel's business)."""
    from smilify_amd import imageprep

    case = CASES.cases()["a_strong"]
    K, K_new, dist = case["lens"]
    tables = imageprep._lens("a_strong", K, dist, K_new, 3, torch.device("cpu"))
    assert all(np.array_equal(got.numpy(), want) for got, want in zip(tables, (K, K_new, dist)))
    uv = np.array([IR.source_coordinate(j, i, case["affine"][0], tuple(t[n] for t in case["lens"]))
                   for n in range(3) for i in range(17) for j in range(17)])
    finite = np.isfinite(uv).all(axis=1)
    inside = finite & (uv[:, 0] > 0) & (uv[:, 0] < 20) & (uv[:, 1] > 0) & (uv[:, 1] < 12)
    assert inside.any() and (finite & ~inside).any() and np.isinf(uv).any() and np.isnan(uv).any()
    assert (finite & (np.abs(uv) > 2.0**31).any(axis=1)).any()  # finite, but beyond what an int holds


# ---- argument checks (no GPU is touched: each raises before the device is asked for) ----
def _good():
    return dict(src=torch.zeros(2, 6, 7, 3, dtype=torch.uint8), size=(4, 5), affine=torch.tensor([[1.0, 0.0, 1.0, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("change,match", [
    (dict(src=torch.zeros(2, 6, 7, 5, dtype=torch.uint8)), "channels"),
    (dict(src=torch.zeros(2, 6, 7, 3, dtype=torch.float64)), "uint8 or float32"),
    (dict(src=torch.zeros(6, 7, dtype=torch.float32)), "uint8 or float32 tensor"),
    (dict(src=torch.zeros(0, 6, 7, 3, dtype=torch.uint8)), "bad source sizes"),
    (dict(size=(0, 5)), "bad output size"),
    (dict(size=(65536, 65536)), "bad output size"),
    (dict(affine=torch.zeros(1, 4, dtype=torch.float32)), "affine"),
    (dict(affine=torch.zeros(1, 3, dtype=torch.float64)), "affine"),
    (dict(affine=torch.zeros(0, 4, dtype=torch.float64)), "affine"),
    (dict(affine=None), "affine is required"),
    (dict(coord_mode="nearest"), "coord_mode"),
    (dict(interpolation="cubic"), "interpolation"),
    (dict(coord_mode="resize_linear", interpolation="nearest"), "goes with"),
    (dict(coord_mode="resize_nearest", interpolation="bilinear"), "goes with"),
    (dict(K=torch.zeros(1, 3, 3, dtype=torch.float64)), "come together"),
    (dict(K=torch.eye(3, dtype=torch.float64), K_new=torch.eye(3, dtype=torch.float64), dist=torch.zeros(4, dtype=torch.float64)), "dist"),
    (dict(K=torch.zeros(2, 3, 3, dtype=torch.float64), K_new=torch.zeros(2, 3, 3, dtype=torch.float64),
          dist=torch.zeros(1, 5, dtype=torch.float64)), "same number of rows"),
    (dict(K=torch.eye(3, dtype=torch.float64), K_new=torch.eye(3, dtype=torch.float64), dist=torch.zeros(5, dtype=torch.float64),
          coord_mode="resize_linear"), "lens needs"),
    (dict(clamp=torch.zeros(1, 4, dtype=torch.int64)), "clamp"),
    (dict(border=torch.zeros(1, 2, dtype=torch.float32)), "border"),
    (dict(n_out=-1), "cannot be launched"),
    (dict(size=(64, 64), n_out=2**28), "cannot be launched"),
    (dict(out_dtype=torch.float16), "out_dtype"),
])
def test_warp_images_refuses_bad_arguments(change, match):
    from smilify_amd import engine

    kw = {**_good(), **change}
    src, size, affine = kw.pop("src"), kw.pop("size"), kw.pop("affine")
    with pytest.raises(ValueError, match=match):
        engine.warp_images(src, size, affine, **kw)


def test_image_bounds_refuses_bad_arguments():
    from smilify_amd import engine

    for bad in (torch.zeros(3, 4), torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, 3, 4, 1), np.zeros((1, 3, 4), np.uint8)):
        with pytest.raises(ValueError, match="image_bounds"):
            engine.image_bounds(bad)


def test_wrappers_refuse_bad_arguments():
    from smilify_amd import imageprep as ip

    sil, rgb, joints = np.zeros((6, 7)), np.zeros((6, 7, 3)), np.zeros((4, 2))
    for args in ((np.zeros((6,)), rgb, joints, 8), (sil, np.zeros((6, 7)), joints, 8), (sil, np.zeros((5, 7, 3)), joints, 8),
                 (sil, rgb, np.zeros((4, 3)), 8), (sil, rgb, joints, 0), (sil[None], rgb, joints, 8),
                 (sil.astype(complex), rgb, joints, 8), (sil, np.zeros((6, 7, 5)), joints, 8)):
        with pytest.raises(ValueError, match="crop_to_silhouette"):
            ip.crop_to_silhouette(*args)
    with pytest.raises(ValueError, match="silhouette_windows"):
        ip.silhouette_windows(np.zeros((2, 3, 4, 5, 6)))
    for args in ((np.zeros((6, 7, 3)), 8, "cubic"), (np.zeros((6,)), 8, "linear"), (np.zeros((6, 7, 3)), (0, 4), "linear"),
                 (np.zeros((2, 6, 7, 9)), 8, "linear")):
        with pytest.raises(ValueError, match="resize_images"):
            ip.resize_images(*args)

    K, d = np.eye(3), np.array([-0.2, 0.1, 0.0, 0.0, 0.01])
    frames = np.zeros((2, 6, 7, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="coefficients"):
        ip.undistort_images(frames, K, np.ones(8))
    for args, kw in (((frames, K, np.ones(3)), {}), ((frames, None, d), {}), ((frames, np.eye(4), d), {}), ((frames, K, np.ones((3, 5))), {}),
                     ((frames, K, d), dict(new_K=np.eye(2))), ((frames, K, d), dict(dtype=np.float64)), ((np.zeros((7,)), K, d), {})):
        with pytest.raises(ValueError, match="undistort_images"):
            ip.undistort_images(*args, **kw)

    masks = np.zeros((2, 6, 7), np.uint8)
    win = np.array([1.0, 2.0, 4.0])
    for args, kw in (((frames[0], masks, K, d, win, 8), {}), ((frames, masks[:1], K, d, win, 8), {}), ((frames, masks, K, d, win, 0), {}),
                     ((frames, masks, K, d, np.ones((3, 3)), 8), {}), ((frames, masks, K, d, np.array([1.0, 2.0, 0.0]), 8), {}),
                     ((frames, masks, K, d, np.array([1.0, np.nan, 3.0]), 8), {}), ((frames, masks, K, d, np.ones(4), 8), {}),
                     ((frames, masks, K, d, win, 8), dict(joints_yx=np.zeros((3, 4, 2)))), ((frames, masks, np.eye(4), d, win, 8), {})):
        with pytest.raises(ValueError, match="prepare_targets"):
            ip.prepare_targets(*args, **kw)
    with pytest.raises(NotImplementedError):
        ip.prepare_targets(frames, masks, K, np.ones(14), win, 8)


def test_zero_distortion_returns_the_input_object():
    from smilify_amd import imageprep as ip

    frames = np.zeros((2, 6, 7, 3), np.uint8)
    for d in (None, [], np.zeros(5), np.full(5, 1e-9), np.zeros((2, 5)), torch.zeros(5)):
        assert ip.undistort_images(frames, np.eye(3), d) is frames
    t = torch.zeros(2, 6, 7)
    assert ip.undistort_images(t, None, None) is t


def test_c_entry_points_refuse_what_they_cannot_index():
    from smilify_amd import _lib

    lib = _lib.load()
    assert lib.smil_image_bounds(None, 1, 1, 0, 4, None, None) == -1 and b"bad sizes" in lib.smil_last_error()
    assert lib.smil_image_bounds(None, 1, 1, 65536, 32768, None, None) == -1 and b"32-bit pixel index" in lib.smil_last_error()
    assert lib.smil_image_bounds(None, 1, 1 << 24, 4096, 4096, None, None) == -1 and b"exceed the grid" in lib.smil_last_error()
    assert lib.smil_image_bounds(None, 1, 2, 4, 4, None, None) == -1 and b"null argument" in lib.smil_last_error()
    assert lib.smil_image_bounds(None, 1, 0, 4, 4, None, None) == 0
    assert lib.smil_warp_images(None, None) == -1

    def warp(**kw):
        w = _lib.Warp()
        w.N_src, w.H, w.W, w.C, w.N, w.S_h, w.S_w, w.n_affine, w.n_border, w.interp = 1, 4, 4, 3, 1, 4, 4, 1, 1, 1
        for k, v in kw.items():
            setattr(w, k, v)
        rc = lib.smil_warp_images(ctypes.byref(w), None)
        return rc, lib.smil_last_error()

    for kw, msg in ((dict(C=5), b"1 .. 4"), (dict(H=0), b"bad sizes"), (dict(coord_mode=3), b"coordinate mode"), (dict(interp=2), b"interpolation"),
                    (dict(coord_mode=1, interp=0), b"its own interpolation"), (dict(K=1), b"come together"), (dict(n_affine=0), b"at least one row"),
                    (dict(K=1, K_new=1, dist=1, n_lens=1, coord_mode=2, interp=0), b"exact coordinate mode"),
                    (dict(clamp=1, n_clamp=0), b"at least one row"), (dict(S_h=65536, S_w=32768), b"32-bit pixel index"),
                    (dict(N=1 << 20, S_h=4096, S_w=4096), b"exceed the grid"), (dict(), b"null argument")):
        rc, err = warp(**kw)
        assert rc == -1 and msg in err, (kw, err)
    assert warp(N=0)[0] == 0
