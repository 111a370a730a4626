"""The warp cases that tests/test_gpu_imageprep_kernels.py runs on the GPU against tests/imageprep_ref.py, as plain data, so that
tests/test_imageprep_cpu.py (and the fixture generator) can assert their premises without one: every case is small enough for the
per-pixel restatement, and no nearest sample of a case with a lens lies within 1e-9 px of a rounding boundary."""
import numpy as np

SEED = 123
SIZES = (5, 8, 17)

# lenses of the 13 x 21 and the 16 x 16 source: moderate barrel distortion with tangential terms, and coefficients so strong that
# some coordinates leave the image, some pass 2^31, some overflow to +-inf and some become NaN
K_A = np.array([[17.5, 0.0, 10.25], [0.0, 18.25, 6.375], [0.0, 0.0, 1.0]])
K_B = np.array([[14.0, 0.0, 7.75], [0.0, 13.5, 8.25], [0.0, 0.0, 1.0]])
DIST_MODERATE = np.array([-0.31, 0.12, 0.013, -0.021, -0.04])
# (three images: coordinates that leave the image; a K_new of focal length 1e-60, under which r2^3 overflows - x radial is +-inf,
# and NaN = 0 inf in the principal point's row and column -; coordinates far beyond 2^31 that stay finite)
DIST_STRONG = np.array([[30.0, 0.0, 0.7, -0.3, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0], [1.0e12, 0.0, 0.0, 0.0, 0.0]])
K_TINY = np.array([[1.0e-60, 0.0, 10.0], [0.0, 1.0e-60, 6.0], [0.0, 0.0, 1.0]])


def sources():
    rng = np.random.default_rng(SEED)
    return {
        "a": rng.integers(0, 256, (3, 13, 21, 3)).astype(np.uint8),          # W no multiple of 4, C = 3
        "b": rng.uniform(-1.0, 1.0, (3, 16, 16, 1)).astype(np.float32),
        "b3": rng.uniform(0.0, 1.0, (3, 16, 16)).astype(np.float32),         # no channel axis
    }


def window_affine(windows, S):
    """exact-mode affine rows of windows (x0, y0, side): output pixel j shows x0 + j side / S."""
    w = np.atleast_2d(np.asarray(windows, np.float64))
    return np.stack([w[:, 2] / S, w[:, 0], w[:, 2] / S, w[:, 1]], axis=1)


# windows of the 13 x 21 source: wholly inside, overhanging the left / top / right / bottom edge, wholly outside, fractional
WINDOWS_A = {
    "inside": (4.0, 2.0, 8.0), "left": (-5.0, 1.0, 10.0), "top": (3.0, -6.0, 9.0), "right": (15.0, 2.0, 11.0), "bottom": (6.0, 8.0, 9.0),
    "outside": (30.0, -40.0, 7.0), "fractional": (2.3, 1.7, 8.5),
}


def cases():
    """name -> dict(src, size, affine, lens, border, scale, planar, n_out): the arguments of imageprep_ref.warp / engine.warp_images."""
    out = {}

    def add(name, src, S, windows, lens=None, border=None, scale=1.0, planar=False, n_out=None):
        out[name] = dict(src=src, size=S, affine=window_affine(windows, S), lens=lens, border=border, scale=scale, planar=planar,
                         n_out=n_out)

    for k, (name, w) in enumerate(WINDOWS_A.items()):  # every window case, the sizes in turn, one image and a shared table
        add(f"a_{name}", "a", SIZES[k % 3], [w], border=[[255.0, 0.0, 128.0]], n_out=1 if k % 2 else 3)
    add("a_per_image", "a", 8, [WINDOWS_A["inside"], WINDOWS_A["left"], WINDOWS_A["fractional"]], border=[[1.0, 2.0, 3.0]] * 3, planar=True,
        scale=1.0 / 255.0)
    lens_a = lambda d: (K_A[None], K_A[None], d[None])  # noqa: E731
    add("a_moderate", "a", 17, [(0.0, -4.0, 21.0)], lens=lens_a(DIST_MODERATE), border=[[255.0, 255.0, 255.0]], scale=1.0 / 255.0, planar=True)
    add("a_moderate_fractional", "a", 8, [WINDOWS_A["fractional"]], lens=lens_a(DIST_MODERATE), n_out=1)
    add("a_strong", "a", 17, [(2.0, -2.0, 17.0)], lens=(np.stack([K_A] * 3), np.stack([K_A, K_TINY, K_A]), DIST_STRONG), border=[[9.0, 8.0, 7.0]])
    K_new = K_B.copy()
    K_new[0, 0], K_new[1, 1], K_new[0, 2] = 11.0, 12.5, 7.25
    per = np.stack([DIST_MODERATE, 0.5 * DIST_MODERATE, np.zeros(5)])
    add("b_per_image_lens", "b", 5, [(0.0, 0.0, 16.0), (3.0, 2.0, 9.0), (-2.5, 4.25, 12.0)],
        lens=(np.stack([K_B] * 3), np.stack([K_new, K_B, K_B]), per), border=[[-2.0]], planar=True)
    add("b_strong", "b", 17, [(0.0, 0.0, 16.0)], lens=(K_B[None], K_B[None], DIST_STRONG[:1]), border=[[0.25]], scale=-3.0)
    add("b3_inside", "b3", 8, [(2.0, 3.0, 11.0)], n_out=1)
    add("b3_moderate", "b3", 17, [(-1.0, -1.0, 18.0)], lens=(K_B[None], K_B[None], DIST_MODERATE[None]), border=[[0.5]])
    return out


def lens_cases():
    return {k: c for k, c in cases().items() if c["lens"] is not None}


def run(warp, case, interpolation, srcs=None):
    srcs = sources() if srcs is None else srcs
    return warp(srcs[case["src"]], case["size"], case["affine"], coord_mode="exact", interpolation=interpolation, lens=case["lens"],
                border=case["border"], scale=case["scale"], planar=case["planar"], n_out=case["n_out"])


def nearest_margin(case):
    """The least distance, over the samples of a case that could read a pixel (within one pixel of the image), of a nearest sample's
    coordinate from the boundary between two taps (k + 0.5), per axis; imageprep_ref.source_coordinate is the map."""
    import imageprep_ref as IR

    src = sources()[case["src"]]
    H, W = src.shape[1:3]
    S = case["size"]
    affine = case["affine"]
    n_out = case["n_out"] or max(len(src), len(affine), len(case["lens"][0]) if case["lens"] else 1)
    best = np.inf
    for n in range(n_out):
        lens = None if case["lens"] is None else tuple(t[n % len(t)] for t in case["lens"])
        for i in range(S):
            for j in range(S):
                u, v = IR.source_coordinate(j, i, affine[n % len(affine)], lens)
                for c, size in ((u, W), (v, H)):
                    if np.isfinite(c) and -2.0 < c < size + 1.0:
                        best = min(best, abs(c + 0.5 - np.floor(c + 0.5) - 0.0), abs(np.floor(c + 0.5) + 1.0 - (c + 0.5)))
    return best
