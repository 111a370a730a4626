"""GPU tests of the two image preparation kernels (``pytest -m gpu``): ``engine.image_bounds`` exactly against numpy and
``engine.warp_images`` against the per-pixel float64 restatement (tests/imageprep_ref.py) on the cases of tests/imageprep_cases.py.

Tolerances.  Nearest results are exact: the tap of a pixel is decided by a float64 coordinate that the kernel forms without
contraction, exactly as the restatement does, and tests/test_imageprep_cpu.py asserts that with a lens no sample lies within 1e-9 px
of a rounding boundary - no pixel is left out.  Bilinear results: ``|d| <= 2e-6 M`` with M the largest tap magnitude
(255 for the bytes, 1 for the float sources; a border value counts as a tap).  The kernel and the restatement use the same float64
coordinates and the same float32 fraction; what remains is fewer than a dozen float32 roundings of size 2^-24 M (three lerps of three
operations each, and the scale), about 7e-7 M, should a compiler contract one of them.  A float64 contraction difference in the
coordinate would move a value by about 1e-13 M.

M is a magnitude of the SOURCE, and the compared values are outputs, taken after the output scale.  Where ``|scale| < 1`` (the
1/255 of byte frames) the roundings shrink with the values, so the bound is taken after the scale too, ``2e-6 M |scale|``: 2e-6 M
would say nothing about outputs in [0, 1].  Where ``|scale| >= 1`` the bound stays 2e-6 M as stated and is NOT widened by the scale:
``2e-6 M min(1, |scale|)`` in every case, never more than 2e-6 M.
"""
import numpy as np
import pytest
import torch

import imageprep_cases as CASES
import imageprep_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BILINEAR_RTOL = 2e-6

t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731


@pytest.fixture(scope="module")
def srcs():
    return CASES.sources()


def _masks(rng, N, H, W, dtype):
    m = (rng.uniform(size=(N, H, W)) < 0.08).astype(dtype)
    if dtype == np.float32:
        m *= rng.uniform(0.01, 3.0, m.shape).astype(np.float32)
        m[rng.uniform(size=m.shape) < 0.05] = -1.0     # negative values and NaN are background
        m[rng.uniform(size=m.shape) < 0.02] = np.nan
    else:
        m *= rng.integers(1, 256, m.shape).astype(np.uint8)
    m[0, H // 2, W // 2] = 1
    m[1] = 0                                            # one mask of the batch is empty
    return m


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shape", [(4, 1, 1), (5, 13, 21), (3, 70, 130), (2, 300, 257)])
def test_image_bounds_is_exact(shape, dtype):
    """1 x 1, 13 x 21, 70 x 130 (more than one wave per row, more than one wave per workgroup) and 300 x 257 (77100 pixels: two slabs
    of one image, which meet by integer atomics), one mask of every batch empty; twice, for the same bits."""
    from smilify_amd import engine

    rng = np.random.default_rng(sum(shape))
    m = _masks(rng, *shape, dtype)
    if shape[1] == 300:
        m[0] = 0
        m[0, 299, 3] = m[0, 2, 256] = 1              # one pixel in each slab only
    want = IR.bounds(np.nan_to_num(m, nan=0.0))
    got = engine.image_bounds(t(m))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    assert torch.equal(engine.image_bounds(t(m)), got)
    empty = want[:, 4] == 0
    assert empty.any() and (~empty).any()
    assert np.array_equal(want[empty][:, :4], np.tile([shape[1], -1, shape[2], -1], (int(empty.sum()), 1)))


def test_image_bounds_of_the_fixture_masks(golden):
    from smilify_amd import engine

    fx = golden("imageprep_ref")
    for g in ("a", "b"):
        for dtype in (np.uint8, np.float32):
            sil = fx[f"{g}_sil"] if dtype == np.float32 else np.ceil(fx[f"{g}_sil"])
            assert np.array_equal(engine.image_bounds(t(sil.astype(dtype))).cpu().numpy(), fx[f"{g}_bounds"]), (g, dtype)
        assert np.array_equal(engine.image_bounds(t(fx[f"{g}_onepx_sil"][None].astype(np.float32))).cpu().numpy(), fx[f"{g}_onepx_bounds"])


def _engine_warp(srcs, case, interpolation, **kw):
    from smilify_amd import engine

    lens = case["lens"]
    return engine.warp_images(t(srcs[case["src"]]), case["size"], t(case["affine"]), interpolation=interpolation,
                              K=None if lens is None else t(lens[0]), K_new=None if lens is None else t(lens[1]),
                              dist=None if lens is None else t(lens[2]),
                              border=None if case["border"] is None else t(np.asarray(case["border"], np.float32)),
                              scale=case["scale"], planar=case["planar"], n_out=case["n_out"], **kw)


def _tap_magnitude(srcs, case):
    m = float(np.abs(srcs[case["src"]].astype(np.float64)).max())
    return max(m, 255.0 if srcs[case["src"]].dtype == np.uint8 else 1.0, float(np.abs(case["border"]).max()) if case["border"] is not None else 0.0)


@pytest.mark.parametrize("name", sorted(CASES.cases()))
def test_warp_against_the_restatement(name, srcs):
    """Every case in both interpolations: windows inside, over each edge, outside, fractional; N = 1 and 3; shared and per-image
    tables; uint8 x 3 channels, float32 x 1 and a source without a channel axis; both layouts; the output scale; lenses from moderate
    to non-finite.  Nearest: equal.  Bilinear: the bound derived in this module's docstring."""
    case = CASES.cases()[name]
    for interpolation in ("nearest", "bilinear"):
        want = CASES.run(IR.warp, case, interpolation, srcs)
        got = _engine_warp(srcs, case, interpolation)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, (got.shape, want.shape)
        got = got.cpu().numpy()
        assert np.isfinite(want).all()
        if interpolation == "nearest":
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        else:
            bound = BILINEAR_RTOL * _tap_magnitude(srcs, case) * min(1.0, abs(case["scale"]))
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{name}: bilinear max |d| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (name, err, bound)
    if name == "a_outside":  # wholly outside: nothing but the border
        assert np.array_equal(got, np.broadcast_to(np.asarray(case["border"], np.float32)[0], got.shape))


def test_warp_uint8_output(srcs):
    """out_dtype uint8 is rint of the clipped float result (computed here from the kernel's own float output)."""
    case = dict(CASES.cases()["a_moderate"], scale=1.7, planar=False)
    f = _engine_warp(srcs, case, "bilinear").cpu().numpy()
    u = _engine_warp(srcs, case, "bilinear", out_dtype=torch.uint8)
    assert u.dtype == torch.uint8 and (f > 255.0).any()
    assert np.array_equal(u.cpu().numpy(), np.rint(np.clip(f, 0.0, 255.0)).astype(np.uint8))


@pytest.mark.parametrize("S", CASES.SIZES)
def test_resize_modes_against_the_restatement(S, srcs):
    """The two cv2.resize modes with per-image rectangles, some reaching past the image (the clamp replicates the RECTANGLE's edge,
    what lies outside the image reads the border): nearest equal, linear to the bilinear bound."""
    from smilify_amd import engine

    rect = np.array([[2, 9, 1, 8], [-3, 6, 4, 15], [12, 20, 9, 12]], np.int32)  # x_lo, x_hi, y_lo, y_hi
    w, h = rect[:, 1] - rect[:, 0] + 1, rect[:, 3] - rect[:, 2] + 1
    affine = np.stack([1.0 / ((S + 1) / w), rect[:, 0].astype(np.float64), 1.0 / (S / h), rect[:, 2].astype(np.float64)], axis=1)
    border = np.array([[7.0, 250.0, 99.0]], np.float32)
    for mode, interp in (("resize_nearest", "nearest"), ("resize_linear", "bilinear")):
        want = IR.warp(srcs["a"], (S, S + 1), affine, mode, interp, clamp=rect, border=border)
        got = engine.warp_images(t(srcs["a"]), (S, S + 1), t(affine), coord_mode=mode, interpolation=interp, clamp=t(rect), border=t(border))
        got = got.cpu().numpy()
        assert got.shape == want.shape == (3, S, S + 1, 3)
        if interp == "nearest":
            assert np.array_equal(got, want)
        else:
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"resize_linear S={S}: max |d| {err:.3e}")
            assert err <= BILINEAR_RTOL * 255.0
        assert (want == border[0]).all(axis=-1).any() and not (want == border[0]).all()
