"""Cost of the target image preparation at camera-frame sizes: ``engine.warp_images`` as ``imageprep.prepare_targets`` uses it (uint8 RGB
frames through a lens and a crop window to planar float32 targets, bilinear) and as ``imageprep.undistort_images`` uses it (the whole
frame, same size out), and ``engine.image_bounds`` on the masks.  After warm-up each call is timed with device events next to a
device-to-device copy of the SAME number of bytes (the bytes the call must move: every source byte a window can touch once, every
output byte once), and one JSON line per workload is printed: ms per call, bytes moved per second, and the copy's.

The events bracket the whole Python call on an idle device (each call follows a synchronize): the argument checks, the allocation of
the output and the launch latency of the host are inside every figure - tens of microseconds, which count against the kernel on the
shorter calls - and ``copy_`` is timed the same way.  The figures are a ceiling on the kernels' own time, not a kernel trace.

    python3 tools/imageprep_probe.py
    python3 tools/imageprep_probe.py --workload crop_1080p --reps 20
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import _lib, engine  # noqa: E402

# frames of one launch; window side in source pixels (None: the whole frame, undistorted at its own size); target size
WORKLOADS = {
    "crop_1080p": dict(N=512, H=1080, W=1920, side=600, S=256),
    "crop_720p": dict(N=1024, H=720, W=1280, side=400, S=256),
    "undistort_1080p": dict(N=128, H=1080, W=1920, side=None, S=None),
    "undistort_1080p_planar": dict(N=128, H=1080, W=1920, side=None, S=None, planar=True),   # the same map, planar output
    "resample_1080p": dict(N=128, H=1080, W=1920, side=None, S=None, lens=False),           # the same taps without the lens arithmetic
    "bounds_1080p": dict(N=512, H=1080, W=1920, side=None, S=None, bounds=True),
}

ap = argparse.ArgumentParser()
ap.add_argument("--workload", action="append", choices=sorted(WORKLOADS))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
dev = torch.device("cuda:0")
version = _lib.load().smil_version().decode()


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total = 0.0
    for it in range(args.warmup + args.reps):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            total += ev[0].elapsed_time(ev[1])
        del out
    return total / args.reps


for name in args.workload or sorted(WORKLOADS):
    w = WORKLOADS[name]
    N, H, W = w["N"], w["H"], w["W"]
    gen = torch.Generator(device="cpu").manual_seed(7)
    if w.get("bounds"):
        masks = (torch.rand(N, H, W, generator=gen) < 0.1).to(torch.uint8).to(dev)
        moved = masks.numel() + N * 20
        ms = timed(lambda: engine.image_bounds(masks))
        scratch = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    else:
        frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
        K = torch.tensor([[[0.9 * W, 0.0, 0.5 * W - 7.0], [0.0, 0.9 * W, 0.5 * H + 4.0], [0.0, 0.0, 1.0]]], dtype=torch.float64, device=dev)
        dist = torch.tensor([[-0.28, 0.09, 0.001, -0.002, -0.01]], dtype=torch.float64, device=dev)
        if w["side"] is None:
            size, affine = (H, W), np.array([[1.0, 0.0, 1.0, 0.0]])
            src_bytes, planar = N * H * W * 3, bool(w.get("planar"))
        else:
            S, side = w["S"], float(w["side"])
            rng = np.random.default_rng(7)
            x0, y0 = rng.uniform(0, W - side, N), rng.uniform(0, H - side, N)
            step = np.full(N, side / S)
            affine = np.stack([step, x0 + 0.5 * (step - 1.0), step, y0 + 0.5 * (step - 1.0)], axis=1)
            size, src_bytes, planar = (S, S), int(N * side * side * 3), True
        affine = torch.from_numpy(affine).to(dev)
        border = torch.full((1, 3), 255.0, dtype=torch.float32, device=dev)
        out_bytes = N * size[0] * size[1] * 3 * 4
        moved = src_bytes + out_bytes
        lens = dict(K=K, K_new=K, dist=dist) if w.get("lens", True) else {}
        ms = timed(lambda: engine.warp_images(frames, size, affine, border=border, scale=1.0 / 255.0, planar=planar, n_out=N, **lens))
        scratch = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(scratch)  # a copy reads and writes: moved / 2 bytes each way are `moved` bytes of traffic
    copy_ms = timed(lambda: dst.copy_(scratch))
    print(json.dumps({"workload": name, "images": N, "H": H, "W": W, "side": w["side"], "S": w["S"], "reps": args.reps, "version": version,
                      "ms": round(ms, 4), "bytes_moved": int(moved), "GB_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
                      "copy_ms": round(copy_ms, 4), "copy_GB_per_s": round(moved / (copy_ms * 1e-3) / 1e9, 1),
                      "images_per_s": round(N / (ms * 1e-3), 1)}), flush=True)
    torch.cuda.empty_cache()
