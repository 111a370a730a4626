"""Times of the mesh hierarchy (smilify_amd.mesh3d.MeshBVH, csrc/mesh_bvh.hip) against the brute force it reproduces
(``mesh3d.closest_points``, csrc/point_mesh.hip) in the same run, on the three workloads of tools/point_mesh_probe.py:
(a) ``model_3000``: 3000 surface samples against the mouse model's mesh; (b) ``hull_model_verts``: the model's vertices against the
hull mesh of a 256^3 carve; (c) ``hull_100k``: 100 000 points around that hull mesh.

Variants, all the whole Python call: ``brute_force`` (closest_points), ``bvh_unsorted`` and ``bvh_sorted`` (MeshBVH.closest_points with
the queries in the caller's order and in Morton order), ``build`` (MeshBVH(meshes): codes, the stable sort, order and boxes) and
``refit``.  Also recorded: the mean and largest number of leaf faces evaluated per point, whether all three answers have equal bits,
and the number of queries after which a build has paid for itself, build / (brute force - bvh).

Needs a GPU; writes profiles/mesh_bvh_probe.json (``--out``).  Every workload is one STEP under its own time limit
(``--step-seconds``), and the variants' windows alternate: the runner and the method are those of tools/probelib.py.  Here: a window
holds 3 to 2000 calls, sized from a first window of 3.  Nothing here is asserted by a test.

    python3 tools/mesh_bvh_probe.py
"""
import argparse
import os
import sys

import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["model_3000", "hull_model_verts", "hull_100k"]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_bvh_probe.json"))
ap.add_argument("--window-ms", type=float, default=300.0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--grid", type=int, default=256, help="lattice of the carve whose hull mesh (b) and (c) use")
ap.add_argument("--step-seconds", type=float, default=240.0, help="time limit of one step (a child process)")
ap.add_argument("--step", choices=STEPS, help="(internal) run this step in this process and print its row")
args = ap.parse_args()


def run_step(name):
    import torch

    sys.path.insert(0, REPO)
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
    trees = {False: mesh3d.MeshBVH(meshes, sort_queries=False), True: mesh3d.MeshBVH(meshes, sort_queries=True)}
    spare = mesh3d.MeshBVH(meshes)

    variants = dict(brute_force=lambda: mesh3d.closest_points(meshes, points),
                    bvh_unsorted=lambda: trees[False].closest_points(points),
                    bvh_sorted=lambda: trees[True].closest_points(points),
                    build=lambda: mesh3d.MeshBVH(meshes),
                    refit=lambda: spare.refit(meshes))
    probelib.warm_up(variants.values(), args.warmup)
    times, calls = probelib.alternate(variants, window_ms=args.window_ms, windows=args.windows, first=3, lo=3, hi=2000)
    row = dict(workload=name, points=P, faces=F, verts=int(verts.shape[0]), leaf_size=int(engine._lib.BVH_LEAF), calls=calls)
    for who, t in times.items():
        row.update({f"{who}_{k}": v for k, v in t.items()})
    for who in ("bvh_unsorted", "bvh_sorted"):
        row[f"brute_force_over_{who}"] = row["brute_force_ms"] / row[f"{who}_ms"]
        # beyond the spread: the slowest window of the hierarchy is still faster than the fastest of the brute force
        row[f"{who}_faster_beyond_spread"] = row[f"{who}_ms_max"] < row["brute_force_ms_min"]
        saved = row["brute_force_ms"] - row[f"{who}_ms"]
        row[f"{who}_queries_to_repay_a_build"] = row["build_ms"] / saved if saved > 0 else None
    count = trees[False].evaluated(points).float()
    row["evaluated_faces_per_point_mean"], row["evaluated_faces_per_point_max"] = float(count.mean()), int(count.max())
    want = variants["brute_force"]()
    row["equal_bits"] = all(torch.equal(a, b) for who in ("bvh_unsorted", "bvh_sorted") for a, b in zip(variants[who](), want))
    probelib.emit_row(row)
    probelib.emit_device([torch.cuda.get_device_name(0), engine._lib.load().smil_version().decode()])


if args.step:
    run_step(args.step)
    sys.exit(0)

forward = ["--window-ms", str(args.window_ms), "--windows", str(args.windows), "--warmup", str(args.warmup), "--grid", str(args.grid)]
rows, failed, device, finished = probelib.run_steps(os.path.abspath(__file__), STEPS, forward, args.step_seconds)
result = dict(device=device and device[0], library=device and device[1], dtype="float32",
              baseline="mesh3d.closest_points (the brute force of csrc/point_mesh.hip) in the same run, alternating windows",
              window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, grid=args.grid, failed=failed,
              not_measured=STEPS[finished:], rows=rows)
probelib.write_result(args.out, result)
sys.exit(1 if failed else 0)
