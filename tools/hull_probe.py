"""Times of the visual hull's kernels (csrc/visual_hull.hip) - carve, statistics, surface count, surface write, each on its own - and of
the same carve in a plain torch formulation (float64 broadcast projection plus an index gather, chunked over the voxels so that its
(chunk, views) temporaries fit), the baseline a user would otherwise write.

Shapes: (N=1, 128^3, 18 views), (N=64, 64^3, 18 views), (N=1, 256^3, 64 views), masks 256^2 (a disc per view: the hull of a camera ring
around it is a rounded blob in the middle of the grid).  Needs a GPU; writes profiles/visual_hull_probe.json (``--out``).  Method: every
path is warmed up (``--warmup`` calls) at every shape; each timed call stands between two device events and ends in a synchronise;
``--repeats`` calls per path, the paths alternating; median, min and max are recorded, the carve's rate in voxel x views per second, the
ratio to the torch baseline and the voxels on which the two disagree (float64 on both sides: expected 0 away from pixel edges).

    python3 tools/hull_probe.py
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import _lib, engine  # noqa: E402
from smilify_amd.cameras import look_at_view_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "visual_hull_probe.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--torch-chunk", type=int, default=1 << 18, help="voxels per chunk of the torch baseline")
ap.add_argument("--shapes", type=str, nargs="*", default=["1,128,18", "64,64,18", "1,256,64"], help="N,G,views")
ap.add_argument("--mask-size", type=int, default=256)
args = ap.parse_args()
dev = torch.device("cuda:0")
ZNEAR = float(torch.tensor(0.001, dtype=torch.float32))


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def torch_carve(masks, cams, S, origin, voxel, G, min_views, max_misses, chunk):
    """occ (N,G,G,G) uint8 by broadcasting: float64 projection of a chunk of voxel centres into every view, an index gather, the vote."""
    N, Nv, H, W = masks.shape
    R, T = cams.R.double(), cams.T.double()  # (Nv,3,3), (Nv,3)
    k11 = 1.0 / torch.tan(cams.fov.double() * 0.017453292519943295 / 2.0)
    hS = 0.5 * S
    vox = G ** 3
    occ = torch.empty(N, vox, dtype=torch.uint8, device=dev)
    flat = masks.reshape(N, Nv, H * W)
    for n in range(N):
        for v0 in range(0, vox, chunk):
            lin = torch.arange(v0, min(vox, v0 + chunk), device=dev)
            idx = torch.stack([lin % G, (lin // G) % G, lin // (G * G)], dim=1).double()
            X = origin + (idx + 0.5) * voxel                                    # (P,3)
            view = torch.einsum("pi,vij->vpj", X, R) + T[:, None, :]            # (Nv,P,3)
            z = view[..., 2]
            ys = hS - hS * (view[..., 1] * k11[:, None] / z)
            xs = hS - hS * (view[..., 0] * k11[:, None] / z)
            seen = (z > ZNEAR) & (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
            pix = torch.where(seen, ys.floor() * W + xs.floor(), torch.zeros_like(ys)).long()
            fg = seen & (torch.gather(flat[n], 1, pix) > 0)
            s, f = seen.sum(0), fg.sum(0)
            occ[n, v0:v0 + lin.numel()] = ((s >= min_views) & (s - f <= max_misses)).to(torch.uint8)
    return occ.reshape(N, G, G, G)


rows = []
for shape in args.shapes:
    N, G, views = (int(x) for x in shape.split(","))
    S = args.mask_size
    az = torch.linspace(0, 360, views + 1)[:views] + 7.3
    el = 20.0 * torch.sin(torch.arange(views) * 2.399) + 5.0
    R, T = look_at_view_transform(2.7, el.numpy(), az.numpy(), device=dev)
    cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 30.0, device=dev), None, views, S)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev) + 0.5, torch.arange(S, device=dev) + 0.5, indexing="ij")
    disc = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.36 * S) ** 2).to(torch.uint8)
    masks = disc[None, None].expand(N, views, S, S).contiguous()
    voxel = 1.4137 / G
    origin = torch.tensor([-0.7137, -0.6911, -0.7023], dtype=torch.float64)
    spec = engine.HullGridSpec(N, (G, G, G), origin, voxel)
    min_views, max_misses = views, 0
    lib = _lib.load()
    ws = torch.empty(int(lib.smil_hull_surface_workspace_bytes(ctypes.byref(spec.struct))), dtype=torch.uint8, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    ptr, stream = engine._ptr, engine._stream

    occ = engine.hull_carve(spec, masks, cams, min_views, max_misses)[0]
    _lib.check(lib.smil_hull_surface_count(ctypes.byref(spec.struct), ptr(occ), ptr(offsets), ptr(ws), stream()))
    total = int(offsets[-1].item())
    points = torch.empty(max(total, 1), 3, dtype=torch.float32, device=dev)
    index = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    paths = {
        "carve": lambda: engine.hull_carve(spec, masks, cams, min_views, max_misses)[0],
        "carve_counts": lambda: engine.hull_carve(spec, masks, cams, min_views, max_misses, want_counts=True)[0],
        "stats": lambda: engine.hull_stats(spec, occ),
        "surface_count": lambda: _lib.check(lib.smil_hull_surface_count(ctypes.byref(spec.struct), ptr(occ), ptr(offsets), ptr(ws), stream())),
        "surface_write": lambda: _lib.check(lib.smil_hull_surface_write(ctypes.byref(spec.struct), ptr(occ), ptr(ws), ptr(points), ptr(index),
                                                                        stream())),
        "torch_carve": lambda: torch_carve(masks, cams, S, origin.to(dev), voxel, G, min_views, max_misses, args.torch_chunk),
    }
    if total == 0:
        del paths["surface_write"]
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in paths.items():
            times[k].append(timed(fn)[0])
    mismatch = int((paths["torch_carve"]() != occ).sum().item())
    row = dict(N=N, grid=G, views=views, mask=S, voxels=N * G ** 3, occupied=int(occ.sum().item()), surface=total, torch_mismatches=mismatch,
               torch_chunk=args.torch_chunk)
    for k, t in times.items():
        row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(t), min(t), max(t)
    row["carve_voxel_views_per_s"] = N * G ** 3 * views / (row["carve_ms"] * 1e-3)
    row["torch_over_carve"] = row["torch_carve_ms"] / row["carve_ms"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    del occ, points, index, masks

out = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smil_version().decode(), repeats=args.repeats, warmup=args.warmup, rows=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
