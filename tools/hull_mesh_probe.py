"""Times of the hull's mesh extraction (csrc/hull_mesh.hip) - ``VisualHull.extract_mesh`` with 0 and with 10 relaxation steps, split into
the count call (classify + scan: the pass that streams the volume) and the write call (emit, relax, finish: surface-sized) - next to
``surface_points()`` on the same hull, the yardstick: it streams the same volume once and packs a surface-sized output.

Shapes: a hull carved from 18 disc views (a ball with facets) in 64^3, 128^3 and 256^3 voxels, N = 1 and N = 16 frames.  Needs a GPU; writes
profiles/hull_mesh_probe.json (``--out``).  Method: every path is warmed up (``--warmup`` calls) at every shape; each timed call stands
between two device events and ends in a synchronise; ``--repeats`` calls per path, the paths alternating; median, min and max are
recorded.  The whole calls include their one host synchronisation (the totals) and their allocations; the split calls run on buffers
allocated beforehand.  Vertex and face counts and the workspace and scratch bytes are recorded with them.

    python3 tools/hull_mesh_probe.py
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import _lib, engine, visual_hull  # noqa: E402
from smilify_amd.cameras import look_at_view_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hull_mesh_probe.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=10, help="relaxation steps of the relaxed paths (Taubin pairs: steps / 2)")
ap.add_argument("--shapes", type=str, nargs="*", default=["1,64", "16,64", "1,128", "16,128", "1,256", "16,256"], help="N,G")
ap.add_argument("--views", type=int, default=18)
ap.add_argument("--mask-size", type=int, default=256)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = _lib.load()
ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def carved(N, G):
    S, views = args.mask_size, args.views
    yy, xx = torch.meshgrid(torch.arange(S, device=dev) + 0.5, torch.arange(S, device=dev) + 0.5, indexing="ij")
    disc = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.36 * S) ** 2).to(torch.uint8)
    az = torch.linspace(0, 360, views + 1)[:views] + 7.3
    el = 20.0 * torch.sin(torch.arange(views) * 2.399) + 5.0
    R, T = look_at_view_transform(2.7, el.numpy(), az.numpy(), device=dev)
    cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 30.0, device=dev), None, views, S)
    masks = disc[None, None].expand(N, views, S, S).contiguous()
    spec = engine.HullGridSpec(N, (G, G, G), torch.tensor([-0.7137, -0.6911, -0.7023], dtype=torch.float64), 1.4137 / G)
    return visual_hull.VisualHull(engine.hull_carve(spec, masks, cams, views, 0)[0], None, None, spec)


rows = []
for shape in args.shapes:
    N, G = (int(x) for x in shape.split(","))
    hull = carved(N, G)
    spec, occ = hull._spec, hull.occupancy
    grid = ctypes.byref(spec.struct)
    weights = np.asarray(visual_hull.taubin_steps(args.steps // 2), np.float64)
    plain = hull.extract_mesh()
    n_verts, n_faces = int(plain.verts.shape[0]), int(plain.faces.shape[0])
    ws_bytes = int(lib.smil_hull_mesh_workspace_bytes(grid))
    scratch_bytes = [int(lib.smil_hull_mesh_scratch_bytes(n_verts, s)) for s in (0, len(weights))]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(scratch_bytes), dtype=torch.uint8, device=dev)
    offsets = torch.empty(2, N + 1, dtype=torch.int64, device=dev)
    verts, normals = torch.empty(n_verts, 3, device=dev), torch.empty(n_verts, 3, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int64, device=dev)

    def count():
        _lib.check(lib.smil_hull_mesh_count(grid, ptr(occ), ptr(offsets[0]), ptr(offsets[1]), ptr(ws), stream()), "smil_hull_mesh_count")

    def write(w, want_normals=True):
        _lib.check(lib.smil_hull_mesh_write(grid, ptr(occ), ptr(ws), ptr(scratch), n_verts, n_faces, w.ctypes.data if len(w) else None, len(w), ptr(verts),
                                            ptr(normals) if want_normals else None, ptr(faces), stream()), "smil_hull_mesh_write")

    none = weights[:0]
    paths = {
        "surface_points": lambda: hull.surface_points(),
        "extract_mesh": lambda: hull.extract_mesh(),
        "extract_mesh_relaxed": lambda: hull.extract_mesh(tuple(weights)),
        "count": count,
        "write": lambda: write(none),
        "write_no_normals": lambda: write(none, False),
        "write_relaxed": lambda: write(weights),
    }
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in paths.items():
            times[k].append(timed(fn)[0])
    assert torch.equal(verts, hull.extract_mesh(tuple(weights)).verts) and torch.equal(faces, plain.faces)
    surface = int(hull.surface_points()[1][-1].item())
    row = dict(shape=shape, N=N, grid=list(hull.grid), views=args.views, voxels=N * G ** 3, cubes=N * (G + 1) ** 3, occupied=int(occ.sum().item()),
               surface_voxels=surface, vertices=n_verts, faces=n_faces, relax_steps=len(weights), workspace_bytes=ws_bytes,
               scratch_bytes=scratch_bytes[0], scratch_bytes_relaxed=scratch_bytes[1], volume_first_frame=float(plain.volume()[0].item()))
    for k, t in times.items():
        row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(t), min(t), max(t)
    row["count_cubes_per_s"] = row["cubes"] / (row["count_ms"] * 1e-3)
    row["mesh_over_surface_points"] = row["extract_mesh_ms"] / row["surface_points_ms"]
    row["relax_ms_per_step"] = (row["write_relaxed_ms"] - row["write_ms"]) / max(len(weights), 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    del hull, occ, ws, scratch, verts, normals, faces, plain

out = dict(device=torch.cuda.get_device_name(0), library=lib.smil_version().decode(), repeats=args.repeats, warmup=args.warmup, rows=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
