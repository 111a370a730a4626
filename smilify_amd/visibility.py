"""Keypoint self-occlusion against a depth buffer: the reference's ``refine_visibility_with_depth``
(smal_fitter/Unreal2Pytorch3D.py:664-760, called per view at :1558-1580) with the same arguments, for one image or for a whole batch
of images in one kernel launch (``engine.depth_visibility``).

The depth buffer is either the replicAnt depth pass as the reference reads it - uint8, the Euclidean camera-to-surface distance in
channel 0 as ``surface = (r / 255) * depth_max_cm`` - or a float32 distance map such as ``Renderer.render_depth(kind="distance")``
(+inf for background, ``depth_max_cm`` unused).  ``encode_depth_u8`` turns the second into the first.
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine


def encode_depth_u8(dist: torch.Tensor, depth_max: float) -> torch.Tensor:
    """Distance map -> the byte of a depth pass whose decoder is ``surface = (r / 255) * depth_max``:
    ``clip(floor(dist / depth_max * 255 + 0.5), 0, 255)`` as uint8, with +inf (background) -> 255.  Rounding to nearest is this
    project's choice: the encoder belongs to the engine that renders the depth pass and is not part of the reference, which only
    decodes."""
    q = torch.floor(dist.double() / float(depth_max) * 255.0 + 0.5)
    return torch.nan_to_num(q, nan=255.0, posinf=255.0).clamp(0.0, 255.0).to(torch.uint8)


def refine_visibility_with_depth(visibility, keypoints_2d_normalized, keypoints_3d_world_raw, camera_location_world_raw, depth_image,
                                 image_width, image_height, depth_max_cm=1000.0, depth_tolerance_cm=5.0, depth_neighborhood=1):
    """Reference Unreal2Pytorch3D.py:664-760.  A keypoint's visibility becomes 0 when its distance to the camera exceeds the
    front-most surface distance over a ``(2 depth_neighborhood + 1)^2`` window around its pixel by more than ``depth_tolerance_cm``;
    it never becomes non-zero.  Keypoints already at 0, without a finite 3-D position, or outside ``[0, 1]^2`` are skipped.

    One image, as the reference: ``visibility`` (P,), ``keypoints_2d_normalized`` (P,2) = (row / H, column / W) - the reference's
    swapped convention -, ``keypoints_3d_world_raw`` (P,3), ``camera_location_world_raw`` (3,), ``depth_image`` (H,W,C) uint8 or
    (H,W) float32 distances: numpy in, numpy out, ``visibility`` refined in place and returned.  A batch: the same with a leading
    axis B on every argument (``camera_location_world_raw`` (B,3), ``depth_image`` (B,H,W,C) uint8 or (B,H,W) float32), arrays or
    tensors; all images go through one launch and a new (B,P) array / tensor of ``visibility``'s kind is returned.

    The early returns are the reference's: ``depth_image`` None, of the wrong rank or of another size than ``image_height`` x
    ``image_width`` leaves ``visibility`` as it is.  ``depth_neighborhood`` above 8 raises."""
    if depth_image is None:
        return visibility
    batched = np.ndim(visibility) == 2
    is_float = (depth_image.dtype == torch.float32) if isinstance(depth_image, torch.Tensor) else (np.asarray(depth_image).dtype == np.float32)
    rank = depth_image.ndim - (1 if batched else 0)
    if is_float:
        if rank != 2:
            return visibility
    elif rank != 3 or depth_image.shape[-1] < 1:
        return visibility
    h0 = 1 if batched else 0
    if depth_image.shape[h0] != image_height or depth_image.shape[h0 + 1] != image_width:
        return visibility

    is_tensor = isinstance(visibility, torch.Tensor)
    dev = torch.device("cuda", torch.cuda.current_device()) if not isinstance(depth_image, torch.Tensor) or depth_image.device.type != "cuda" \
        else depth_image.device

    def dev_of(a, dtype):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        t = t.to(device=dev, dtype=dtype)
        return t if batched else t[None]

    depth = dev_of(depth_image, torch.float32 if is_float else torch.uint8)
    kp_norm = dev_of(keypoints_2d_normalized, torch.float64)
    cam = dev_of(camera_location_world_raw, torch.float64)
    kp_dist = (dev_of(keypoints_3d_world_raw, torch.float64) - cam[:, None]).norm(dim=-1)  # (NaN for a keypoint without a 3-D position)
    vis = dev_of(visibility, torch.float32)
    out = engine.depth_visibility(depth, kp_norm.contiguous(), kp_dist.contiguous(), vis.contiguous(), float(depth_tolerance_cm),
                                  max(int(depth_neighborhood), 0), depth_max=float(depth_max_cm))
    if batched:
        if is_tensor:
            return out.to(device=visibility.device, dtype=visibility.dtype)
        return out.cpu().numpy().astype(np.asarray(visibility).dtype, copy=False)
    if is_tensor:
        visibility.copy_(out[0].to(device=visibility.device, dtype=visibility.dtype))
    else:
        visibility[...] = out[0].cpu().numpy()
    return visibility
