"""Writes tests/golden/visibility_ref.npz by running the REFERENCE's ``refine_visibility_with_depth``
(smal_fitter/Unreal2Pytorch3D.py:664-760) on generated depth buffers and keypoints (build container only; data only - inputs and the
visibilities the reference returns, nothing of its text).

    python tests/golden/make_visibility_fixture.py

The module is imported the way make_golden.py imports the fitter (``install_stubs`` for ``config``, ``nibabel`` and ``pytorch3d``), with
empty stub modules for the packages it names at import time that are absent here.

Two groups of images - ``a``: 3 images of 12 x 20 x 4 bytes, depth_max 1000, tolerance 5; ``b``: 3 images of 16 x 16 x 1, depth_max
437.5, tolerance 2.25 - each run with depth_neighborhood 0, 1 and 2 on keypoints of its own (the threshold depends on the window).
Per image and neighbourhood, in this order:

* keypoints at norm exactly 0.0 and 1.0 in every combination with each other and with an interior coordinate (windows clipped at
  every corner and every edge), far behind the surface;
* keypoints outside [0, 1] on each of the four sides, and with a NaN coordinate on either axis (skipped);
* a keypoint without a 3-D position (NaN) and one whose visibility is 0 coming in, both far behind the surface (skipped);
* keypoints over a pixel of byte 0 and over a window whose bytes are all 255;
* random interior keypoints clearly in front of and clearly behind the threshold;
* keypoints whose distance is ``(surface + tolerance) (1 +- e)`` for e = 1e-6, 1e-7, 1e-8, 1e-9, 1e-10: what float32 cannot decide.

The generator asserts that no keypoint lies within 1e-12 (relative) of its threshold - so none has to be left out of a comparison for
being undecidable in float64 - and that the test-side restatement (tests/fragments_ref.py) returns what the reference returns; the
``surface`` arrays are the restatement's (the reference does not hand its sample out).
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (first: it puts the repository root on the path)
import fragments_ref as FR  # noqa: E402

SEED = 77
GROUPS = {"a": dict(H=12, W=20, C=4, depth_max=1000.0, tolerance=5.0), "b": dict(H=16, W=16, C=1, depth_max=437.5, tolerance=2.25)}
IMAGES, NEIGHBORHOODS = 3, (0, 1, 2)
EPSILONS = (1e-6, 1e-7, 1e-8, 1e-9, 1e-10)
ABSENT = ["cv2", "imageio", "pycocotools", "skimage", "trimesh", "pytorch3d"]  # packages the module names that are not installed here


class _Stub(types.ModuleType):
    """An absent package: any name imported from it is None (the function under test uses none of them)."""

    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Answers every import below the absent packages with a ``_Stub``."""

    def find_spec(self, name, path=None, target=None):
        return importlib.machinery.ModuleSpec(name, self, is_package=True) if name.split(".")[0] in ABSENT else None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def reference_function():
    make_golden.install_stubs(make_golden.MODELS["stick"])
    for name in [k for k in sys.modules if k.split(".")[0] in ABSENT]:  # (install_stubs names only what the fitter imports)
        del sys.modules[name]
    sys.meta_path.append(_StubFinder())
    from smal_fitter.Unreal2Pytorch3D import refine_visibility_with_depth
    return refine_visibility_with_depth


def depth_image(rng, H, W, C):
    img = rng.integers(20, 236, (H, W, C)).astype(np.uint8)
    r, c = int(rng.integers(3, H - 3)), int(rng.integers(3, W - 3))
    img[r - 2:r + 3, c - 2:c + 3, 0] = 255                # a 5 x 5 block at depth_max (a whole window of 255 for every neighbourhood)
    while True:                                           # one pixel at distance 0, outside the block
        zr, zc = int(rng.integers(H)), int(rng.integers(W))
        if abs(zr - r) > 2 or abs(zc - c) > 2:
            break
    img[zr, zc, 0] = 0
    return img, (r, c)


def keypoints(rng, img, block, h, depth_max, tolerance):
    """(norm (P,2), points (P,3), camera (3,), visibility (P,)) of one image for half-window h."""
    H, W = img.shape[:2]
    cam = rng.uniform(-300.0, 300.0, 3)
    norm, dist, vis, nan3 = [], [], [], []

    def threshold(nx, ny):
        one = np.array([1.0], np.float32)
        _, s = FR.visibility_rules(one, [(nx, ny)], [0.0], img, h, tolerance, depth_max)
        return s[0] + tolerance

    def add(nx, ny, d, v=1.0, nan_point=False):
        norm.append((nx, ny)); dist.append(d); vis.append(v); nan3.append(nan_point)

    far = 3.0 * depth_max
    inner = lambda n: (rng.integers(1, n - 1) + rng.uniform(0.2, 0.8)) / n  # noqa: E731
    for nx in (0.0, 1.0):                      # corners
        for ny in (0.0, 1.0):
            add(nx, ny, far)
    for e in (0.0, 1.0):                       # edges
        add(e, inner(W), far)
        add(inner(H), e, far)
    for nx, ny in ((-0.01, 0.5), (1.01, 0.5), (0.5, -0.01), (0.5, 1.01), (np.nan, 0.5), (0.5, np.nan)):
        add(nx, ny, far)
    add(inner(H), inner(W), far, nan_point=True)
    add(inner(H), inner(W), far, v=0.0)
    zr, zc = np.argwhere(img[..., 0] == 0)[0]
    add((zr + 0.5) / H, (zc + 0.5) / W, tolerance * 0.5)          # over byte 0: in front of the tolerance
    add((zr + 0.5) / H, (zc + 0.5) / W, tolerance * 1.5)          # ... and behind it
    add((block[0] + 0.5) / H, (block[1] + 0.5) / W, depth_max + 0.5 * tolerance)   # a window of 255 only
    add((block[0] + 0.5) / H, (block[1] + 0.5) / W, depth_max + 1.5 * tolerance)
    for k in range(6):                          # clearly decided
        nx, ny = inner(H), inner(W)
        add(nx, ny, threshold(nx, ny) * (0.7 if k % 2 else 1.3))
    for e in EPSILONS:                          # what float32 cannot decide
        for sign in (-1.0, 1.0):
            nx, ny = inner(H), inner(W)
            add(nx, ny, threshold(nx, ny) * (1.0 + sign * e))
    norm, dist = np.asarray(norm, np.float64), np.asarray(dist, np.float64)
    u = rng.normal(size=(len(dist), 3))
    pts = cam + dist[:, None] * u / np.linalg.norm(u, axis=1, keepdims=True)
    pts[np.asarray(nan3), 1] = np.nan
    return norm, pts, cam, np.asarray(vis, np.float32)


def main():
    ref = reference_function()
    rng = np.random.default_rng(SEED)
    out, total, near = {}, 0, 0
    for g, cfg in GROUPS.items():
        H, W, C, depth_max, tol = cfg["H"], cfg["W"], cfg["C"], cfg["depth_max"], cfg["tolerance"]
        images = [depth_image(rng, H, W, C) for _ in range(IMAGES)]
        depth = np.stack([im for im, _ in images])
        out[f"{g}_depth"], out[f"{g}_depth_max"], out[f"{g}_tolerance"] = depth, np.float64(depth_max), np.float64(tol)
        for h in NEIGHBORHOODS:
            per = [keypoints(rng, im, blk, h, depth_max, tol) for im, blk in images]
            norm, pts, cam, vis = (np.stack([p[k] for p in per]) for k in range(4))
            got = np.stack([ref(vis[b].copy(), norm[b], pts[b], cam[b], depth[b], W, H, depth_max_cm=depth_max, depth_tolerance_cm=tol,
                                depth_neighborhood=h) for b in range(IMAGES)])
            mine, surface = FR.refine_visibility_batch(vis, norm, pts, cam, depth, h, tol, depth_max)
            assert np.array_equal(mine, got), (g, h)
            d = FR.point_distances(pts, cam)
            with np.errstate(invalid="ignore"):
                rel = np.abs(d - (surface + tol)) / (surface + tol)
            assert not (rel < 1e-12).any(), (g, h, float(np.nanmin(rel)))
            near += int((rel < 1.5e-6).sum())
            total += vis.size
            for k, v in dict(norm=norm, points=pts, camera=cam, vis_in=vis, vis_out=got.astype(np.float32), surface=surface).items():
                out[f"{g}_h{h}_{k}"] = v
    path = os.path.join(HERE, "visibility_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {total} keypoints, {near} within 1.5e-6 of their threshold, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
