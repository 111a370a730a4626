"""float64 numpy restatement of the target image preparation (smilify_amd/csrc/imageprep.hip, semantics at include/smilfit.h and
DESIGN.md section 4.11): per-pixel loops, float64 coordinates, float32 exactly where the kernel is specified to round - the
resize_linear coordinate, the bilinear fraction and the three lerps of the blend.  Nothing here is vectorised and nothing is shared
with the product."""
import math

import numpy as np

F32 = np.float32
LIMIT = 1073741824.0  # 2^30: where a finite coordinate beyond it is moved (every tap there is outside any image)


def bounds(sil):
    """(N,H,W) -> (N,5) int32 y_min, y_max, x_min, x_max, count over pixels > 0; H, -1, W, -1, 0 without one."""
    sil = np.asarray(sil)
    N, H, W = sil.shape
    out = np.zeros((N, 5), np.int32)
    for n in range(N):
        ys, xs = np.nonzero(sil[n] > 0)
        out[n] = (ys.min(), ys.max(), xs.min(), xs.max(), ys.size) if ys.size else (H, -1, W, -1, 0)
    return out


def windows_from_bounds(b, margin=1.05):
    """crop_to_silhouette's square (smal_fitter/utils.py:26-28) in its own integer arithmetic, on the unpadded image: (x0, y0, side)."""
    out = np.zeros((len(b), 3), np.float64)
    for n, (y_min, y_max, x_min, x_max, _) in enumerate(np.asarray(b).tolist()):
        half = int(margin * (max(x_max - x_min, y_max - y_min) / 2))
        cy, cx = y_min + int((y_max - y_min) / 2), x_min + int((x_max - x_min) / 2)
        out[n] = (cx - half, cy - half, 2 * half)
    return out


def distort(K, K_new, d, u, v):
    """cv2.undistort's map as documented: pixel (u, v) of camera K_new -> pixel of the distorted camera K."""
    k1, k2, p1, p2, k3 = (float(c) for c in d)
    with np.errstate(all="ignore"):
        u, v = np.float64(u), np.float64(v)
        x, y = (u - K_new[0][2]) / K_new[0][0], (v - K_new[1][2]) / K_new[1][1]
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)
        xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x))
        yd = y * radial + p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y
        return K[0][0] * xd + K[0][2], K[1][1] * yd + K[1][2]


def source_coordinate(j, i, affine, lens=None):
    """exact mode: the float64 source coordinate (u, v) of output column j, row i."""
    ax, bx, ay, by = (np.float64(a) for a in affine)
    u, v = ax * np.float64(j) + bx, ay * np.float64(i) + by
    if lens is not None:
        u, v = distort(lens[0], lens[1], lens[2], u, v)
    return float(u), float(v)


def _exact_tap(u, bilinear):
    """(first tap, float32 fraction, finite)"""
    if not math.isfinite(u):
        return 0, F32(0), False
    u = min(max(u, -LIMIT), LIMIT)
    if bilinear:
        f = math.floor(u)
        return int(f), F32(np.float64(u) - np.float64(f)), True
    return int(math.floor(u + 0.5)), F32(0), True


def _resize_tap(j, a, b, linear):
    origin = float(b)
    if linear:
        f = F32(np.float64(j + 0.5) * np.float64(a) - np.float64(0.5))
        fl = F32(np.floor(f))
        return int(origin + float(fl)), F32(f - fl), True
    return int(origin + math.floor(np.float64(j) * np.float64(a))), F32(0), True


def _lerp(a, b, w):
    return F32(a + F32(w * F32(b - a)))


def warp(src, size, affine, coord_mode="exact", interpolation="bilinear", lens=None, clamp=None, border=None, scale=1.0, planar=False,
         n_out=None):
    """src (N_src,H,W,C) or (N_src,H,W); affine (k,4); lens = (K (k,3,3), K_new (k,3,3), dist (k,5)) or None; clamp (k,4) ints or None;
    border (k,C) or None (zeros).  float32 (N,S_h,S_w,C) (no channel axis for a 3-D src) or planar (N,C,S_h,S_w)."""
    src = np.asarray(src)
    has_c = src.ndim == 4
    if not has_c:
        src = src[..., None]
    N_src, H, W, C = src.shape
    S_h, S_w = (size, size) if np.ndim(size) == 0 else size
    affine = np.asarray(affine, np.float64).reshape(-1, 4)
    border = np.zeros((1, C), F32) if border is None else np.asarray(border, F32).reshape(-1, C)
    clamp = None if clamp is None else np.asarray(clamp, np.int64).reshape(-1, 4)
    if lens is not None:
        lens = [np.asarray(t, np.float64) for t in lens]
        lens = [lens[0].reshape(-1, 3, 3), lens[1].reshape(-1, 3, 3), lens[2].reshape(-1, 5)]
    N = n_out if n_out is not None else max([N_src, len(affine), len(border)] + ([len(clamp)] if clamp is not None else [])
                                            + ([len(lens[0])] if lens is not None else []))
    bilinear = interpolation == "bilinear"
    scale = F32(scale)
    out = np.zeros((N, S_h, S_w, C), F32)
    for n in range(N):
        img, af, bd = src[n % N_src], affine[n % len(affine)], border[n % len(border)]
        ln = None if lens is None else tuple(t[n % len(t)] for t in lens)
        rect = None if clamp is None else clamp[n % len(clamp)]

        def tap(x, y, c):
            return F32(img[y, x, c]) if 0 <= x < W and 0 <= y < H else bd[c]

        for i in range(S_h):
            for j in range(S_w):
                if coord_mode == "exact":
                    u, v = source_coordinate(j, i, af, ln)
                    x0, wx, okx = _exact_tap(u, bilinear)
                    y0, wy, oky = _exact_tap(v, bilinear)
                else:
                    x0, wx, okx = _resize_tap(j, af[0], af[1], coord_mode == "resize_linear")
                    y0, wy, oky = _resize_tap(i, af[2], af[3], coord_mode == "resize_linear")
                x1, y1 = x0 + 1, y0 + 1
                if rect is not None:
                    x0, x1 = (int(min(max(x, rect[0]), rect[1])) for x in (x0, x1))
                    y0, y1 = (int(min(max(y, rect[2]), rect[3])) for y in (y0, y1))
                for c in range(C):
                    if not (okx and oky):
                        a = b = cc = d = bd[c]
                    else:
                        a = tap(x0, y0, c)
                        if bilinear:
                            b, cc, d = tap(x1, y0, c), tap(x0, y1, c), tap(x1, y1, c)
                    if bilinear:
                        val = _lerp(_lerp(a, b, wx), _lerp(cc, d, wx), wy)
                    else:
                        val = a
                    out[n, i, j, c] = F32(val * scale)
    if planar:
        return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
    return out if has_c else out[..., 0]


def resize(img, size, interpolation):
    """cv2.resize of ONE image (H,W) or (H,W,C) to size = (S_w, S_h) - OpenCV's dsize order - with INTER_NEAREST ("nearest") or
    INTER_LINEAR ("linear") in OpenCV's conventions: ifx = 1.0 / (S_w / W) in float64; nearest sx = min(floor(j ifx), W - 1); linear
    fx = float32((j + 0.5) ifx - 0.5), sx = floor(fx), weight fx - sx, sx < 0 -> (0, weight 0), sx >= W - 1 -> (W - 1, weight 0).
    The result keeps img's dtype where it is a float type (the reference passes float64 arrays), computed in float32."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    S_w, S_h = size
    ifx, ify = 1.0 / (S_w / W), 1.0 / (S_h / H)
    mode = "resize_nearest" if interpolation == "nearest" else "resize_linear"
    out = warp(img[None].astype(F32), (S_h, S_w), [[ifx, 0.0, ify, 0.0]], coord_mode=mode,
               interpolation="nearest" if interpolation == "nearest" else "bilinear", clamp=[[0, W - 1, 0, H - 1]])[0]
    return out.astype(img.dtype) if img.dtype.kind == "f" else out


def crop_to_silhouette(sil_img, rgb_img, joints, target_size):
    """The whole of smal_fitter/utils.py:7-49 through the warp: (sil (S,S), rgb (S,S,3), joints (J,2)), float32 images."""
    sil_img, rgb_img = np.asarray(sil_img), np.asarray(rgb_img)
    x0, y0, side = windows_from_bounds(bounds(sil_img[None]))[0]
    S = target_size
    ifx = 1.0 / (S / side)
    rect = [[int(x0), int(x0 + side - 1), int(y0), int(y0 + side - 1)]]
    af = [[ifx, x0, ifx, y0]]
    sil = warp(sil_img[None].astype(F32), S, af, "resize_nearest", "nearest", clamp=rect, border=[[0.0]])[0]
    rgb = warp(rgb_img[None].astype(F32), S, af, "resize_linear", "bilinear", clamp=rect, border=[[1.0] * rgb_img.shape[2]])[0]
    joints = np.asarray(joints)
    scaled = np.zeros_like(joints)
    scaled[:, 0] = joints[:, 0] - y0
    scaled[:, 1] = joints[:, 1] - x0
    return sil, rgb, scaled * (S / side)
