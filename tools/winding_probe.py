"""Times of the winding numbers (smilify_amd.mesh3d.winding_number, k_pm_winding of csrc/point_mesh.hip) on the workloads of
tools/point_mesh_probe.py, next to ``closest_points`` (k_pm_points: the same traffic, comparable arithmetic) on the same inputs in the
same run, and to a float32 torch brute force of the same formula (tests/winding_ref.py's pair values, all pairs, chunked over the
points so that it fits, then the sum), all on the same device.

Workloads: (a) ``model_3000``: 3000 points around the mouse model's mesh; (b) ``hull_model_verts``: the model's vertices against the
hull mesh of a 256^3 carve (``VisualHull.extract_mesh``) - the containment question; (c) ``hull_100k``: 100 000 points around that hull
mesh against it.  The torch brute force is timed on at most ``--torch-points`` of the points; its time per point is what the ratio
compares, and the row says how many points it ran.

Needs a GPU; writes profiles/winding_probe.json (``--out``).  Every workload is one STEP under its own time limit
(``--step-seconds``), and the variants' windows alternate: the runner and the method are those of tools/probelib.py.  Here: a window
holds 3 to 2000 calls, sized from a first window of 3.  Nothing here is asserted by a test, and no time is a gate.

    python3 tools/winding_probe.py
"""
import argparse
import datetime
import os
import sys

import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["model_3000", "hull_model_verts", "hull_100k"]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "winding_probe.json"))
ap.add_argument("--window-ms", type=float, default=300.0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--grid", type=int, default=256, help="lattice of the carve whose hull mesh (b) and (c) use")
ap.add_argument("--torch-points", type=int, default=1024)
ap.add_argument("--step-seconds", type=float, default=240.0, help="time limit of one step (a child process)")
ap.add_argument("--step", choices=STEPS, help="(internal) run this step in this process and print its row")
args = ap.parse_args()


def run_step(name):
    import torch

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import winding_ref as ref
    from smilify_amd import engine, fit3d, mesh3d, model_io, visual_hull
    from smilify_amd.cameras import look_at_view_transform
    from smilify_amd.mesh3d import Meshes

    dev = torch.device("cuda:0")

    def hull_mesh(G):  # a disc seen by 18 cameras, carved (tools/point_mesh_probe.py's scene)
        S, views = 256, 18
        yy, xx = torch.meshgrid(torch.arange(S, device=dev) + 0.5, torch.arange(S, device=dev) + 0.5, indexing="ij")
        disc = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.36 * S) ** 2).to(torch.uint8)
        az = torch.linspace(0, 360, views + 1)[:views] + 7.3
        el = 20.0 * torch.sin(torch.arange(views) * 2.399) + 5.0
        R, T = look_at_view_transform(2.7, el.numpy(), az.numpy(), device=dev)
        cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 30.0, device=dev), None, views, S)
        spec = engine.HullGridSpec(1, (G, G, G), torch.tensor([-0.7137, -0.6911, -0.7023], dtype=torch.float64), 1.4137 / G)
        occ = engine.hull_carve(spec, disc[None, None].expand(1, views, S, S).contiguous(), cams, views, 0)[0]
        m = visual_hull.VisualHull(occ, None, None, spec).extract_mesh(return_normals=False)
        return m.verts.float().contiguous(), m.faces.long().contiguous()

    t = model_io.load_model(os.path.join(REPO, "data", "models", "SMILy_Mouse_static_joints.npz"))
    mv = torch.from_numpy(t.v_template).float().to(dev)
    mv = (mv - mv.mean(0)) / (mv - mv.mean(0)).abs().max() * 0.45  # inside the carve's volume
    mf = torch.from_numpy(t.faces.astype("int64")).to(dev)
    g = torch.Generator().manual_seed(1)
    if name == "model_3000":
        verts, faces = mv, mf
        points, _ = fit3d.sample_points_with_faces(Meshes([verts], [faces]), 3000, seed=5)
        points = (points + 0.02 * torch.randn(points.shape, generator=g).to(dev)).contiguous()
    else:
        verts, faces = hull_mesh(args.grid)
        if name == "hull_model_verts":
            points = mv[None].contiguous()
        else:
            base = verts[torch.randint(0, len(verts), (100000,), generator=g).to(dev)]
            points = (base + 0.03 * torch.randn(base.shape, generator=g).to(dev))[None].contiguous()
    meshes = Meshes([verts], [faces])
    P, F = int(points.shape[1]), int(faces.shape[0])
    tp = min(P, args.torch_points)
    tri = verts[faces]
    v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    nrm = torch.linalg.cross(e1, e2)

    def winding():
        return mesh3d.winding_number(meshes, points)

    def closest():
        return engine.point_mesh_distance(verts, meshes.face_tables(), points)

    def torch_brute():
        chunk = max(1, min(tp, (1 << 24) // F))
        return torch.cat([ref._pair_values(torch, v0, e1, e2, nrm, points[0, s:min(s + chunk, tp), None, :]).sum(1) for s in range(0, tp, chunk)])

    variants = dict(winding_number=winding, closest_points_kernels=closest, torch_brute_force=torch_brute)
    probelib.warm_up(variants.values(), args.warmup)
    times, calls = probelib.alternate(variants, window_ms=args.window_ms, windows=args.windows, first=3, lo=3, hi=2000)
    row = dict(workload=name, points=P, faces=F, verts=int(verts.shape[0]), torch_points=tp, calls=calls)
    for who, t in times.items():
        row.update({f"{who}_{k}": v for k, v in t.items()})
    row["winding_over_closest_points"] = row["winding_number_ms"] / row["closest_points_kernels_ms"]
    row["torch_per_point_over_kernel_per_point"] = (row["torch_brute_force_ms"] / tp) / (row["winding_number_ms"] / P)
    row["pairs_per_second"] = P * F / (row["winding_number_ms"] * 1e-3)
    # the same answer: the kernel's numbers against the brute force on the points both ran, and what they say
    w = winding()[0]
    row["max_abs_difference_to_torch"] = float((w[:tp] - torch_brute()).abs().max())
    row["share_inside"] = float((w > 0.5).double().mean())
    row["largest_distance_to_an_integer"] = float((w - w.round()).abs().max())
    probelib.emit_row(row)
    probelib.emit_device([torch.cuda.get_device_name(0), engine._lib.load().smil_version().decode()])


if args.step:
    run_step(args.step)
    sys.exit(0)

forward = ["--window-ms", str(args.window_ms), "--windows", str(args.windows), "--warmup", str(args.warmup), "--grid", str(args.grid),
           "--torch-points", str(args.torch_points)]
rows, failed, device, finished = probelib.run_steps(os.path.abspath(__file__), STEPS, forward, args.step_seconds)
result = dict(device=device and device[0], library=device and device[1], dtype="float32", date=datetime.date.today().isoformat(),
              baseline="tests/winding_ref.py _pair_values on the device in float32, all pairs, chunked over the points, float sum",
              compared_with="engine.point_mesh_distance (k_pm_extent, k_pm_table, k_pm_points, k_pm_finish) on the same inputs",
              window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, grid=args.grid, failed=failed,
              not_measured=STEPS[finished:], rows=rows)
probelib.write_result(args.out, result)
sys.exit(1 if failed else 0)
