"""Times of the distance-field kernels (csrc/distance_field.hip) - the transform of a carved hull (outside; inside with the border), the
same for a batch of masks (inside without the border), and the sampler with its gradient at P points per frame - and of the transform a user would write today in
torch on the same GPU: ``torch.cdist`` of chunks of voxel indices against the indices of ``surface_points()``, the minimum over the
surface, zero on the occupied voxels (the nearest occupied voxel of an unoccupied one is a surface voxel).

Shapes: the hulls of tools/hull_probe.py - (N=1, 128^3, 18 views), (N=64, 64^3, 18 views), (N=1, 256^3, 64 views), a disc per view - and 256
disc masks of 256^2 as frames of grid (256, 256, 1).  Needs a GPU; writes profiles/distance_field_probe.json (``--out``).  Method: every
path is warmed up (``--warmup`` calls) at every shape; each timed call stands between two device events and ends in a synchronise;
``--repeats`` calls per path, the paths alternating; median, min and max are recorded, the transform's rate in voxels per second, the
ratio to the torch baseline and the voxels on which the baseline's squared distance, rounded, differs from the kernel's ``d2``.

    python3 tools/distance_field_probe.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import _lib, engine, visual_hull  # noqa: E402
from smilify_amd.cameras import look_at_view_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "distance_field_probe.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--points", type=int, default=4096, help="sample points per frame")
ap.add_argument("--torch-bytes", type=float, default=2e9, help="bytes of one (chunk, surface) float32 distance matrix of the baseline")
ap.add_argument("--shapes", type=str, nargs="*", default=["1,128,18", "64,64,18", "1,256,64", "masks,256,256"], help="N,G,views or masks,N,S")
ap.add_argument("--mask-size", type=int, default=256)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def disc(S):
    yy, xx = torch.meshgrid(torch.arange(S, device=dev) + 0.5, torch.arange(S, device=dev) + 0.5, indexing="ij")
    return (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.36 * S) ** 2).to(torch.uint8)


def carved(N, G, views):
    S = args.mask_size
    az = torch.linspace(0, 360, views + 1)[:views] + 7.3
    el = 20.0 * torch.sin(torch.arange(views) * 2.399) + 5.0
    R, T = look_at_view_transform(2.7, el.numpy(), az.numpy(), device=dev)
    cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 30.0, device=dev), None, views, S)
    masks = disc(S)[None, None].expand(N, views, S, S).contiguous()
    spec = engine.HullGridSpec(N, (G, G, G), torch.tensor([-0.7137, -0.6911, -0.7023], dtype=torch.float64), 1.4137 / G)
    return visual_hull.VisualHull(engine.hull_carve(spec, masks, cams, views, 0)[0], None, None, spec)


def mask_frames(N, S):
    occ = disc(S)[None, None].expand(N, 1, S, S).contiguous()
    return visual_hull.VisualHull(occ, None, None, engine.HullGridSpec(N, (S, S, 1), (0.0, 0.0, 0.0), 1.0))


def torch_transform(hull, surface, offsets):
    """d2 (N,Gz,Gy,Gx) int32 by all pairs: chunks of voxel indices against the frame's surface voxel indices."""
    Gx, Gy, Gz = hull.grid
    N, vox = hull.occupancy.shape[0], Gx * Gy * Gz
    out = torch.empty(N, vox, dtype=torch.int32, device=dev)
    for n in range(N):
        surf = surface[offsets[n]:offsets[n + 1]]
        if surf.shape[0] == 0:
            out[n] = _lib.EDT_NONE
            continue
        chunk = max(1, int(args.torch_bytes / (4 * surf.shape[0])))
        for v0 in range(0, vox, chunk):
            lin = torch.arange(v0, min(vox, v0 + chunk), device=dev)
            idx = torch.stack([lin % Gx, (lin // Gx) % Gy, lin // (Gx * Gy)], dim=1).float()
            d = torch.cdist(idx, surf).amin(dim=1)
            out[n, v0:v0 + lin.numel()] = torch.round(d * d).to(torch.int32)
    return torch.where(hull.occupancy.reshape(N, vox) != 0, torch.zeros_like(out), out).reshape(hull.occupancy.shape)


rows = []
for shape in args.shapes:
    kind, a, b = shape.split(",")
    if kind == "masks":
        N, G, views = int(a), int(b), 0
        hull = mask_frames(N, G)
    else:
        N, G, views = int(kind), int(a), int(b)
        hull = carved(N, G, views)
    Gx, Gy, Gz = hull.grid
    _, index, offsets = hull.surface_points(return_index=True)
    surface = torch.stack([index % Gx, (index // Gx) % Gy, index // (Gx * Gy)], dim=1).float()
    offsets = offsets.tolist()
    d2 = hull.distance_transform()
    field = hull.distance_field(signed=True)
    gen = torch.Generator(device=dev).manual_seed(N + G)
    lo = hull.origin.to(dev).float() - 0.1 * G * hull.voxel_size.to(dev).float()
    points = lo + torch.rand(N, args.points, 3, device=dev, generator=gen) * (1.2 * torch.tensor([Gx, Gy, Gz], device=dev) * hull.voxel_size.to(dev).float())
    if kind == "masks":  # the 2-D form: (y, x) points; no border (it would lie one cell above and below every pixel)
        points = points[..., [1, 0]].contiguous()
    paths = {
        "transform": lambda: hull.distance_transform(),
        "transform_inside": lambda: hull.distance_transform(inside=True, border=kind != "masks"),
        "sample": lambda: engine.field_sample(field._spec, field.d2_out, None, points)[0],
        "sample_signed": lambda: engine.field_sample(field._spec, field.d2_out, field.d2_in, points)[0],
        "torch_transform": lambda: torch_transform(hull, surface, offsets),
    }
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in paths.items():
            times[k].append(timed(fn)[0])
    mismatch = int((paths["torch_transform"]() != d2).sum().item())
    row = dict(shape=shape, N=N, grid=list(hull.grid), views=views, voxels=N * Gx * Gy * Gz, occupied=int(hull.occupancy.sum().item()),
               surface=offsets[-1], points_per_frame=args.points, torch_mismatches=mismatch, torch_bytes=args.torch_bytes,
               max_d2=int(d2.max().item()))
    for k, t in times.items():
        row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(t), min(t), max(t)
    row["transform_voxels_per_s"] = row["voxels"] / (row["transform_ms"] * 1e-3)
    row["sample_points_per_s"] = N * args.points / (row["sample_ms"] * 1e-3)
    row["torch_over_transform"] = row["torch_transform_ms"] / row["transform_ms"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    del hull, field, d2, points, surface, index

out = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smil_version().decode(), repeats=args.repeats, warmup=args.warmup, rows=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
