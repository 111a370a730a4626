"""Target image preparation on the GPU: what the reference does on the host, one frame at a time, with OpenCV before a fit -
``cv2.undistort`` per camera frame (smal_fitter/sleap_data/preprocess_sleap_multiview_dataset.py:710-735, :969-1028) and
``crop_to_silhouette`` (smal_fitter/utils.py:7-49) - for whole batches in one kernel launch each (``engine.image_bounds``,
``engine.warp_images``; csrc/imageprep.hip).

* ``silhouette_windows``   the reference's 1.05 x square around every mask, as ``cameras.crop_intrinsics`` windows.
* ``crop_to_silhouette``   the reference function, for one image or a batch: two resizes in OpenCV's conventions.
* ``resize_images``        the same resizes of whole images.
* ``undistort_images``     ``cv2.undistort``'s map, bilinear, border 0.
* ``prepare_targets``      the fused route: undistortion, crop window and resize in ONE resampling; its output is the image of the
                           camera ``cameras.crop_intrinsics(K, window, S)`` / ``cameras.opencv_to_pinhole_camera(R, t, K, S, window)``.

Arrays in, arrays out; tensors in, tensors on the device out (as ``visibility.refine_visibility_with_depth``).  Pixel (column j,
row i) of an image is the sample AT integer coordinate (j, i), OpenCV's convention; DESIGN.md section 4.11 relates it to the
renderer's.  OpenCV itself is not needed and not used: the conventions are restated, parity with ``cv2`` has not been run.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cameras, engine


def _device(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            return x.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")


def _images(who, name, x, channels, batched_ndim):
    """x as a contiguous uint8 / float32 tensor with a leading batch axis (not yet on the device), and whether it had that axis.
    channels: None (no channel axis), or True (a channel axis of 1 .. 4)."""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
        if x.dtype == np.bool_:
            x = x.astype(np.uint8)
        elif x.dtype != np.uint8:
            if x.dtype.kind not in "fiu":
                raise ValueError(f"{who}: {name} must be a numeric image, got dtype {x.dtype}")
            x = x.astype(np.float32)
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif x.dtype == torch.bool:
        x = x.to(torch.uint8)
    elif x.dtype != torch.uint8:
        if not (x.dtype.is_floating_point or x.dtype in (torch.int8, torch.int16, torch.int32, torch.int64)):
            raise ValueError(f"{who}: {name} must be a numeric image, got dtype {x.dtype}")
        x = x.to(torch.float32)
    if x.dim() not in (batched_ndim - 1, batched_ndim):
        what = "(N,H,W,C) or (H,W,C)" if channels else "(N,H,W) or (H,W)"
        raise ValueError(f"{who}: {name} must be {what}, got {tuple(x.shape)}")
    batched = x.dim() == batched_ndim
    if not batched:
        x = x[None]
    if channels and not 1 <= x.shape[-1] <= 4:
        raise ValueError(f"{who}: {name} has {x.shape[-1]} channels, 1 to 4 are supported")
    if min(x.shape) < 1:
        raise ValueError(f"{who}: {name} is empty: {tuple(x.shape)}")
    return x.contiguous(), batched


def _back(t: torch.Tensor, like):
    return t if isinstance(like, torch.Tensor) else t.cpu().numpy()


def _f64(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float64))
    return t.to(device=dev, dtype=torch.float64).contiguous()


def windows_from_bounds(bounds, margin: float = 1.05) -> np.ndarray:
    """``(N,5)`` bounds ``y_min, y_max, x_min, x_max, count`` -> ``(N,3)`` float64 windows ``(x0, y0, side)`` in crop_to_silhouette's
    own integer arithmetic (utils.py:26-28) on the unpadded image: ``half = int(margin * (max(x_max - x_min, y_max - y_min) / 2))``,
    ``centre = min + int((max - min) / 2)``, ``x0 = centre_x - half``, ``y0 = centre_y - half``, ``side = 2 half``.  An empty mask
    (count 0) raises ``ValueError`` naming the images."""
    b = np.asarray(bounds).astype(np.int64)
    if b.ndim != 2 or b.shape[1] != 5:
        raise ValueError(f"windows_from_bounds: bounds must be (N,5), got {b.shape}")
    empty = np.nonzero(b[:, 4] <= 0)[0]
    if empty.size:
        raise ValueError(f"silhouette_windows: no foreground pixel in image(s) {empty.tolist()}")
    out = np.zeros((len(b), 3), np.float64)
    for n, (y_min, y_max, x_min, x_max, _) in enumerate(b.tolist()):
        half = int(margin * (max(x_max - x_min, y_max - y_min) / 2))
        out[n] = (x_min + int((x_max - x_min) / 2) - half, y_min + int((y_max - y_min) / 2) - half, 2 * half)
    return out


def silhouette_windows(sil, margin: float = 1.05):
    """``(bounds (N,5) int32, windows (N,3) float64)`` of masks ``sil`` (N,H,W) (pixels > 0 are foreground): the bounding box by an
    exact integer reduction on the GPU, and ``windows_from_bounds`` of it.  Both are numpy arrays (a window is host data: it goes
    into ``cameras.crop_intrinsics``).  An empty mask raises ``ValueError`` naming the images, as the reference fails on one."""
    s, _ = _images("silhouette_windows", "sil", sil, None, 3)
    bounds = engine.image_bounds(s.to(_device(sil))).cpu().numpy()
    return bounds, windows_from_bounds(bounds, margin)


def _check_windows(who, windows, N):
    w = np.asarray(windows.detach().cpu() if isinstance(windows, torch.Tensor) else windows, dtype=np.float64)
    if w.shape == (3,):
        w = w[None]
    if w.ndim != 2 or w.shape[1] != 3 or w.shape[0] not in (1, N):
        raise ValueError(f"{who}: windows must be (3,) or (k,3) = (x0, y0, side) with k = 1 or {N}, got {w.shape}")
    if not np.isfinite(w).all() or (w[:, 2] <= 0).any():
        bad = np.nonzero(~np.isfinite(w).all(axis=1) | (w[:, 2] <= 0))[0]
        raise ValueError(f"{who}: window(s) {bad.tolist()} are not finite with a positive side")
    if (np.abs(w) >= 2.0**30).any():
        raise ValueError(f"{who}: windows beyond 2^30 pixels")
    return w


def _resize_warp(img, S_hw, windows, linear, border, dev):
    """cv2.resize of the rectangles ``windows`` (k,4) = (x0, y0, width, height) whole source pixels, to S_hw."""
    S_h, S_w = S_hw
    w = np.asarray(windows, np.float64)
    affine = np.stack([1.0 / (S_w / w[:, 2]), w[:, 0], 1.0 / (S_h / w[:, 3]), w[:, 1]], axis=1)
    clamp = np.stack([w[:, 0], w[:, 0] + w[:, 2] - 1, w[:, 1], w[:, 1] + w[:, 3] - 1], axis=1).astype(np.int32)
    C = img.shape[3] if img.dim() == 4 else 1
    return engine.warp_images(img.to(dev), (S_h, S_w), _f64(affine, dev), coord_mode="resize_linear" if linear else "resize_nearest",
                              interpolation="bilinear" if linear else "nearest", clamp=torch.from_numpy(clamp).to(dev),
                              border=torch.full((1, C), float(border), dtype=torch.float32, device=dev))


def crop_to_silhouette(sil_img, rgb_img, joints, target_size):
    """The reference's ``crop_to_silhouette`` (smal_fitter/utils.py:7-49) with its signature and return value - ``sil_img`` (H,W),
    ``rgb_img`` (H,W,3), ``joints`` (J,2) = (y, x), ``target_size`` S -> ``(sil (S,S), rgb (S,S,3), joints (J,2))`` - and the same
    for a batch (a leading axis N on all three).  Images come back float32.

    The square is ``silhouette_windows`` of the mask; where it leaves the image the mask is padded with 0 and the RGB image with 1.
    The mask is resized with INTER_NEAREST and the RGB image with INTER_LINEAR, in OpenCV's conventions for a source of ``side``
    and a destination of ``S`` pixels: ``ifx = 1.0 / (S / side)`` in float64; nearest: ``sx = min(floor(j * ifx), side - 1)``;
    linear: ``fx = float32((j + 0.5) * ifx - 0.5)``, ``sx = floor(fx)``, weight ``fx - sx``, with ``sx < 0`` -> ``(0, weight 0)`` and
    ``sx >= side - 1`` -> ``(side - 1, weight 0)`` (edge replication of the square, not of the image).  The blend runs in float32.
    Joints: ``(joints - (y0, x0)) * (S / side)`` (:42-47).  A mask without foreground, or of a single row and column of it (a square
    of side 0, on which the reference fails inside cv2.resize), raises ``ValueError``."""
    who = "crop_to_silhouette"
    sil, batched = _images(who, "sil_img", sil_img, None, 3)
    rgb, rgb_batched = _images(who, "rgb_img", rgb_img, True, 4)
    if batched != rgb_batched or sil.shape != rgb.shape[:3]:
        raise ValueError(f"{who}: sil_img {tuple(np.shape(sil_img))} and rgb_img {tuple(np.shape(rgb_img))} do not belong together")
    S = int(target_size)
    if S < 1:
        raise ValueError(f"{who}: target_size={target_size}")
    N = sil.shape[0]
    j_t = isinstance(joints, torch.Tensor)
    j_np = joints.detach().cpu().numpy() if j_t else np.asarray(joints)
    if j_np.ndim != (3 if batched else 2) or j_np.shape[-1] != 2 or (batched and j_np.shape[0] != N):
        raise ValueError(f"{who}: joints must be {'(N,J,2)' if batched else '(J,2)'}, got {j_np.shape}")
    dev = _device(sil_img, rgb_img)
    sil = sil.to(dev)
    _, win = silhouette_windows(sil)
    flat = np.nonzero(win[:, 2] <= 0)[0]
    if flat.size:
        raise ValueError(f"{who}: the square of image(s) {flat.tolist()} has side 0")
    rect = np.stack([win[:, 0], win[:, 1], win[:, 2], win[:, 2]], axis=1)
    sil_out = _resize_warp(sil, (S, S), rect, False, 0.0, dev)
    rgb_out = _resize_warp(rgb, (S, S), rect, True, 1.0, dev)
    jb = j_np if batched else j_np[None]
    scaled = np.zeros_like(jb)
    scaled[..., 0] = jb[..., 0] - win[:, None, 1]
    scaled[..., 1] = jb[..., 1] - win[:, None, 0]
    scaled = scaled * (S / win[:, 2])[:, None, None]
    if not batched:
        sil_out, rgb_out, scaled = sil_out[0], rgb_out[0], scaled[0]
    return _back(sil_out, sil_img), _back(rgb_out, rgb_img), (torch.from_numpy(scaled).to(joints.device) if j_t else scaled)


def resize_images(images, size, interpolation: str = "linear"):
    """``cv2.resize`` of whole images, ``(N,H,W,C)``, ``(N,H,W)`` or one ``(H,W,C)`` (a 2-D array is one ``(H,W)`` image), to
    ``size = (S_h, S_w)`` or a square ``S``, with ``interpolation`` "nearest" or "linear" in the conventions stated at
    ``crop_to_silhouette`` (per axis, with the image as the replicated rectangle).  float32 out.

    A 3-D input is read by its last axis alone: 4 or less and it is ONE ``(H,W,C)`` image, more and it is a batch ``(N,H,W)``.  A
    batch of channel-less images 1 to 4 pixels wide must therefore be passed as ``(N,H,W,1)``."""
    who = "resize_images"
    if interpolation not in ("nearest", "linear"):
        raise ValueError(f"{who}: interpolation is 'nearest' or 'linear', got {interpolation!r}")
    nd = np.ndim(images) if not isinstance(images, torch.Tensor) else images.dim()
    if nd == 4 or (nd == 3 and images.shape[-1] <= 4):
        img, batched = _images(who, "images", images, True, 4)
    else:
        img, batched = _images(who, "images", images, None, 3)
    try:
        S_h, S_w = (int(v) for v in size)
    except TypeError:
        S_h = S_w = int(size)
    if S_h < 1 or S_w < 1:
        raise ValueError(f"{who}: size={size}")
    dev = _device(images)
    H, W = int(img.shape[1]), int(img.shape[2])
    out = _resize_warp(img, (S_h, S_w), np.array([[0.0, 0.0, W, H]]), interpolation == "linear", 0.0, dev)
    return _back(out if batched else out[0], images)


def _lens(who, K, dist, new_K, N, dev):
    """(K, K_new, dist) device tables, or None when dist is None, empty or all close to 0 (np.allclose(dist, 0), :990-996)."""
    if dist is None:
        return None
    d = np.asarray(dist.detach().cpu() if isinstance(dist, torch.Tensor) else dist, dtype=np.float64)
    if d.size == 0:
        return None
    if d.ndim == 1:
        d = d[None]
    if d.ndim != 2 or d.shape[0] not in (1, N):
        raise ValueError(f"{who}: dist must be (5,) or (k,5) with k = 1 or {N}, got {d.shape}")
    if d.shape[1] > 5:
        raise NotImplementedError(f"{who}: {d.shape[1]} distortion coefficients; only k1, k2, p1, p2, k3 are supported")
    if d.shape[1] < 5:
        if d.shape[1] != 4:
            raise ValueError(f"{who}: dist must hold 4 or 5 coefficients, got {d.shape[1]}")
        d = np.concatenate([d, np.zeros((d.shape[0], 1))], axis=1)
    if np.allclose(d, 0.0):
        return None
    Ks = []
    for name, k in (("K", K), ("new_K", K if new_K is None else new_K)):
        if k is None:
            raise ValueError(f"{who}: K is required with distortion coefficients")
        k = np.asarray(k.detach().cpu() if isinstance(k, torch.Tensor) else k, dtype=np.float64)
        if k.shape == (3, 3):
            k = k[None]
        if k.ndim != 3 or k.shape[1:] != (3, 3) or k.shape[0] not in (1, N):
            raise ValueError(f"{who}: {name} must be (3,3) or (k,3,3) with k = 1 or {N}, got {k.shape}")
        Ks.append(k)
    rows = max(Ks[0].shape[0], Ks[1].shape[0], d.shape[0])
    grow = lambda t: np.array(np.broadcast_to(t, (rows,) + t.shape[1:]))  # noqa: E731  (a copy: torch wants writable memory)
    return tuple(_f64(grow(t), dev) for t in (Ks[0], Ks[1], d))


def undistort_images(images, K, dist, new_K=None, dtype=None):
    """``cv2.undistort(image, K, dist, None, new_K)`` for ``images`` (N,H,W,C), (N,H,W) or one (H,W,C): every output pixel (u, v) of
    the camera ``new_K`` (default ``K``) shows the source pixel that ``initUndistortRectifyMap`` documents - normalise by ``new_K``,
    apply ``dist = (k1, k2, p1, p2, k3)`` (radial and tangential), back through ``K`` - in float64 per pixel, sampled bilinearly with
    a constant border of 0.  ``K`` / ``new_K`` (3,3) and ``dist`` (5,) or one row per image.  More than five coefficients raise
    ``NotImplementedError`` (as ``triangulate.undistort_points``).  ``dist`` None, empty or all close to 0 returns ``images`` itself,
    unchanged (preprocess_sleap_multiview_dataset.py:990-996).  A 3-D input is read by its last axis alone, as in ``resize_images``:
    4 or less and it is ONE ``(H,W,C)`` image, more and it is a batch ``(N,H,W)``; pass narrower channel-less batches as ``(N,H,W,1)``.

    Returns float32; with ``dtype=np.uint8`` (or ``torch.uint8``) the float result clipped to [0, 255] and rounded to nearest even.
    That is NOT the bytes OpenCV returns: its ``remap`` interpolates uint8 images with 5-bit fixed-point weights."""
    who = "undistort_images"
    if dtype not in (None, np.uint8, np.float32, torch.uint8, torch.float32):
        raise ValueError(f"{who}: dtype must be uint8 or float32")
    nd = np.ndim(images) if not isinstance(images, torch.Tensor) else images.dim()
    if nd == 4 or (nd == 3 and images.shape[-1] <= 4):
        img, batched = _images(who, "images", images, True, 4)
    else:
        img, batched = _images(who, "images", images, None, 3)
    N, H, W = (int(v) for v in img.shape[:3])
    dev = _device(images)
    lens = _lens(who, K, dist, new_K, N, dev)
    if lens is None:
        return images
    affine = torch.tensor([[1.0, 0.0, 1.0, 0.0]], dtype=torch.float64, device=dev)
    out = engine.warp_images(img.to(dev), (H, W), affine, K=lens[0], K_new=lens[1], dist=lens[2],
                             out_dtype=torch.uint8 if dtype in (np.uint8, torch.uint8) else torch.float32)
    return _back(out if batched else out[0], images)


# Where output pixel j of the fused route samples the (undistorted) source, in source pixel indices: x0 + (j + c) side / S - c.
# c = 0.5 is the renderer's convention (csrc/common.h pix_to_ndc, csrc/camera.h ndc_to_yx): pixel j covers [j, j + 1) of the image
# plane and is sampled at its centre j + 0.5, so a source pixel index k stands for the coordinate k + 0.5 of cameras.crop_points_yx.
# c = 0 would read crop_points_yx as a map between pixel INDICES; the two agree for side == S and differ by (side / S - 1) / 2 source
# pixels otherwise, and against the renderer c = 0.5 wins (tests/test_gpu_imageprep.py).
FUSED_CENTRE = 0.5


def prepare_targets(frames, masks, K, dist, windows, S, joints_yx=None):
    """The fused route from camera frames to fitter targets: undistortion, crop window and resize in ONE resampling per image
    (the reference resamples twice: cv2.undistort, then cv2.resize inside crop_to_silhouette).

    ``frames`` (N,H,W,3) uint8 (scaled by 1/255) or float32 (taken as they are); ``masks`` (N,H,W), foreground > 0; ``K`` (3,3) or
    (N,3,3) and ``dist`` (5,) or (N,5) (None or all zero: no lens) of the cameras the frames come from; ``windows`` (3,) or (N,3) =
    ``(x0, y0, side)`` in UNDISTORTED source pixels, fractional and overhanging windows allowed (``silhouette_windows`` of
    undistorted masks, or any tracker's boxes); ``S`` the target size.

    The output is the image of the camera ``cameras.crop_intrinsics(K, window, S)``: output pixel (j, i) shows the undistorted source
    pixel ``(x0 + (j + 0.5) side / S - 0.5, y0 + (i + 0.5) side / S - 0.5)`` - the inverse of ``cameras.crop_points_yx`` between pixel
    CENTRES, the renderer's convention (``FUSED_CENTRE``); ``(x0 + j, y0 + i)`` for ``side == S`` -, which the lens ``dist`` maps into
    the frame as ``undistort_images`` does.  Masks are sampled nearest (``floor(u + 0.5)``) with border 0, frames bilinearly with
    border 1 (the reference's paddings).  Returns ``(rgb (N,3,S,S) float32, sil (N,1,S,S) float32 holding the masks' own values,
    joints_yx cropped with cameras.crop_points_yx or None)``: the ``data_batch`` layout of ``SMALFitter``; with
    ``cameras.opencv_to_pinhole_camera(R, t, K, S, window)`` next to it that is a complete fitter input."""
    who = "prepare_targets"
    rgb, fb = _images(who, "frames", frames, True, 4)
    sil, mb = _images(who, "masks", masks, None, 3)
    if not (fb and mb) or rgb.shape[:3] != sil.shape:
        raise ValueError(f"{who}: frames (N,H,W,C) {tuple(np.shape(frames))} and masks (N,H,W) {tuple(np.shape(masks))} do not belong together")
    N = int(rgb.shape[0])
    S = int(S)
    if S < 1:
        raise ValueError(f"{who}: S={S}")
    win = _check_windows(who, windows, N)
    if joints_yx is not None and (np.ndim(joints_yx) != 3 or joints_yx.shape[0] != N or joints_yx.shape[-1] != 2):
        raise ValueError(f"{who}: joints_yx must be (N,J,2), got {tuple(joints_yx.shape)}")
    dev = _device(frames, masks)
    lens = _lens(who, K, dist, None, N, dev)
    step = win[:, 2] / float(S)
    shift = FUSED_CENTRE * (step - 1.0)
    affine = _f64(np.stack([step, win[:, 0] + shift, step, win[:, 1] + shift], axis=1), dev)
    kw = {} if lens is None else dict(K=lens[0], K_new=lens[1], dist=lens[2])
    C = int(rgb.shape[3])
    white = 255.0 if rgb.dtype == torch.uint8 else 1.0  # (the border is a source value: it is scaled with the taps)
    rgb_out = engine.warp_images(rgb.to(dev), (S, S), affine, interpolation="bilinear", planar=True, n_out=N,
                                 border=torch.full((1, C), white, dtype=torch.float32, device=dev), scale=1.0 / white, **kw)
    sil_out = engine.warp_images(sil.to(dev), (S, S), affine, interpolation="nearest", planar=True, n_out=N, **kw)
    joints = None
    if joints_yx is not None:
        if len(win) == 1:
            joints = cameras.crop_points_yx(joints_yx, win[0], S)
        elif isinstance(joints_yx, torch.Tensor):
            joints = torch.stack([cameras.crop_points_yx(joints_yx[n], win[n], S) for n in range(N)])
        else:
            joints = np.stack([cameras.crop_points_yx(np.asarray(joints_yx)[n], win[n], S) for n in range(N)])
    return _back(rgb_out, frames), _back(sil_out, masks), joints


# ---- distance transforms of masks (csrc/distance_field.hip: every image a frame of grid (W, H, 1)) -------------------------------------
def mask_distance_transform(masks, threshold: float = 0.0, inside: bool = False) -> torch.Tensor:
    """int32, the shape of ``masks`` ((N,Nv,H,W) or (N,H,W), any real dtype or bool, on the GPU): the exact squared distance in pixels from
    every pixel to the nearest pixel ``> threshold`` (a NaN is background, as in ``visual_hull.carve``).  ``inside``: to the nearest
    background pixel instead (the surroundings of the image do not count: an image is one slice of a grid, whose border would lie one
    cell above and below every pixel).  Centre to centre: a target pixel reads 0.  An image without a target reads 2^31 - 1 everywhere.  The kernel is the visual hull's
    ``distance_transform``."""
    if not isinstance(masks, torch.Tensor) or masks.dim() not in (3, 4):
        raise ValueError("masks must be a tensor (N,Nv,H,W) or (N,H,W)")
    dev = engine.require_gpu(masks.device)
    H, W = int(masks.shape[-2]), int(masks.shape[-1])
    fg = ((masks.float() if masks.dtype == torch.bool else masks) > threshold).to(torch.uint8).reshape(-1, 1, H, W)
    spec = engine.HullGridSpec(fg.shape[0], (W, H, 1), (0.0, 0.0, 0.0), 1.0)
    return engine.hull_edt(spec, fg.to(dev), invert=inside).reshape(masks.shape)


class _MaskSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, d2):
        H, W = int(d2.shape[-2]), int(d2.shape[-1])
        spec = engine.HullGridSpec(d2.numel() // (H * W), (W, H, 1), (0.0, 0.0, 0.0), 1.0)
        want = points.requires_grad
        value, grad = engine.field_sample(spec, d2.reshape(spec.shape()), None, points.reshape(spec.N, -1, 2), want_grad=want)
        ctx.save_for_backward(grad) if want else ctx.save_for_backward()
        ctx.want = want
        return value.reshape(points.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        if not ctx.want:
            return None, None
        (grad,) = ctx.saved_tensors
        return g[..., None] * grad.reshape(g.shape + (2,)), None


def sample_mask_distance(d2, points_yx) -> torch.Tensor:
    """float32 ``(..., P)``: the distance in pixels of ``points_yx (..., P, 2)`` - ``(y, x)`` pixels, the project's order - to the
    foreground of the masks whose ``mask_distance_transform`` is ``d2 (..., H, W)`` (the same leading shape), differentiable in the points.
    Pixel ``(r, c)`` covers ``[r, r+1) x [c, c+1)``, its centre lies at ``(r + 0.5, c + 0.5)`` (the convention of ``visual_hull``); the value
    is ``sqrt(d2)`` at a centre, bilinear between centres, and grows by the distance to the box of pixel centres outside it.  Centre to
    centre: a point inside a foreground pixel but off its centre reads a small positive value next to background.  A NaN or infinite
    point reads 0 with gradient 0; an image without foreground reads 0 everywhere."""
    if not (isinstance(d2, torch.Tensor) and isinstance(points_yx, torch.Tensor)) or d2.dim() < 3 or points_yx.dim() != d2.dim() \
            or points_yx.shape[-1] != 2 or points_yx.shape[:-2] != d2.shape[:-2]:
        raise ValueError("sample_mask_distance: d2 (..., H, W) and points_yx (..., P, 2) with the same leading shape")
    return _MaskSampleFn.apply(points_yx, d2)
