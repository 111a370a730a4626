"""Writes tests/golden/imageprep_ref.npz by running the REFERENCE's ``crop_to_silhouette`` (smal_fitter/utils.py:7-49) on generated
masks, images and joints (build container only; data only - inputs and what the reference returns, nothing of its text).

    python tests/golden/make_imageprep_fixture.py

The module is imported the way make_visibility_fixture.py imports its function (``make_golden.install_stubs`` for ``config``, ``cv2``
and ``nibabel``).  OpenCV is not installed here, so the stub's ``cv2.resize`` IS THE RESTATEMENT'S resize (tests/imageprep_ref.py
``resize``, OpenCV's documented conventions).  The fixture therefore records the reference's OWN bounding box, padding, square
and shifted and scaled joints, and its two resizes AS RESTATED; parity with OpenCV's own resize has not been run.

Two groups - ``a``: 13 x 21 pixels, ``b``: 16 x 16 - of three images each:

* a plus-shaped mask that touches all four image edges (in ``a`` the 1.05 x square reaches into the padding above and below);
* an L-shaped mask;
* a tall blob in a corner, whose square overhangs the right edge;

each cropped to ``target_size`` 5, 8 and 17 (down- and up-scaling, odd sides), with an RGB image of float64 values in [0, 1] and four
joints, two of them outside the square.  Per group also a ONE-PIXEL mask: its bounding box has extent 0, the square has side 0 and
the reference fails inside cv2.resize (the stub raises as OpenCV does on an empty source); the fixture records that and the window.

It also asserts what the CPU test asserts again for the warp cases that the GPU tests run with a lens
(tests/imageprep_cases.py): no nearest sample lies within 1e-9 px of a rounding boundary, so no pixel is left out of a comparison.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (first: it puts the repository root on the path)
import imageprep_cases as CASES  # noqa: E402
import imageprep_ref as IR  # noqa: E402

SEED = 91
SIZES = (5, 8, 17)
GROUPS = {"a": (13, 21), "b": (16, 16)}


def reference_function():
    make_golden.install_stubs(make_golden.MODELS["stick"])
    cv2 = sys.modules["cv2"]
    cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1

    def resize(src, dsize, interpolation=1):
        if src.size == 0:
            raise ValueError("resize: empty source (OpenCV: !ssize.empty())")
        return IR.resize(src, dsize, "nearest" if interpolation == cv2.INTER_NEAREST else "linear")

    cv2.resize = resize
    from smal_fitter.utils import crop_to_silhouette
    return crop_to_silhouette


def masks(H, W):
    edges = np.ones((H, W))  # a plus: the corners are background
    for ys in (slice(0, 4), slice(H - 4, H)):
        for xs in (slice(0, 5), slice(W - 5, W)):
            edges[ys, xs] = 0.0
    ell = np.zeros((H, W))
    ell[2:H - 3, 3:5] = 1.0
    ell[H - 5:H - 3, 3:W - 4] = 1.0
    blob = np.zeros((H, W))
    blob[0:9, W - 3:W] = 0.5  # (foreground is > 0, not == 1)
    blob[1, W - 2] = 0.0
    one = np.zeros((H, W))
    one[H // 3, W // 2] = 1.0
    return np.stack([edges, ell, blob]), one


def main():
    ref = reference_function()
    rng = np.random.default_rng(SEED)
    out = {}
    for g, (H, W) in GROUPS.items():
        sil, one = masks(H, W)
        rgb = rng.uniform(0.0, 1.0, (3, H, W, 3))
        joints = np.stack([np.array([[rng.uniform(0, H), rng.uniform(0, W)], [H / 2.0, W / 2.0], [-3.5, W + 2.25], [H + 1.0, -0.5]])
                           for _ in range(3)])
        out[f"{g}_sil"], out[f"{g}_rgb"], out[f"{g}_joints"] = sil, rgb, joints
        out[f"{g}_bounds"] = IR.bounds(sil)
        out[f"{g}_windows"] = IR.windows_from_bounds(out[f"{g}_bounds"])
        for S in SIZES:
            got = [ref(sil[n], rgb[n], joints[n], S) for n in range(3)]
            out[f"{g}_S{S}_sil"], out[f"{g}_S{S}_rgb"], out[f"{g}_S{S}_joints"] = (np.stack([r[k] for r in got]) for k in range(3))
            for n in range(3):  # the reference's square is the window: its joints say so
                x0, y0, side = out[f"{g}_windows"][n]
                np.testing.assert_allclose(got[n][2], (joints[n] - [y0, x0]) * (S / side), rtol=0, atol=1e-12)
        out[f"{g}_onepx_sil"] = one
        out[f"{g}_onepx_bounds"] = IR.bounds(one[None])
        out[f"{g}_onepx_window"] = IR.windows_from_bounds(out[f"{g}_onepx_bounds"])[0]
        try:
            ref(one, rgb[0], joints[0], 8)
            raised = False
        except ValueError:
            raised = True
        out[f"{g}_onepx_reference_raises"] = np.bool_(raised)

    for name, case in CASES.lens_cases().items():
        margin = CASES.nearest_margin(case)
        assert margin > 1e-9, (name, margin)
    path = os.path.join(HERE, "imageprep_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
