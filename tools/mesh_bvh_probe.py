"""Times of the mesh hierarchy (smilify_amd.mesh3d.MeshBVH, csrc/mesh_bvh.hip) against the brute force it reproduces
(``mesh3d.closest_points``, csrc/point_mesh.hip) in the same run, on the three workloads of tools/point_mesh_probe.py:
(a) ``model_3000``: 3000 surface samples against the mouse model's mesh; (b) ``hull_model_verts``: the model's vertices against the
hull mesh of a 256^3 carve; (c) ``hull_100k``: 100 000 points around that hull mesh.

Variants, all the whole Python call: ``brute_force`` (closest_points), ``bvh_unsorted`` and ``bvh_sorted`` (MeshBVH.closest_points with
the queries in the caller's order and in Morton order), ``build`` (MeshBVH(meshes): codes, the stable sort, order and boxes) and
``refit``.  Also recorded: the mean and largest number of leaf faces evaluated per point, whether all three answers have equal bits,
and the number of queries after which a build has paid for itself, build / (brute force - bvh).

Needs a GPU; writes profiles/mesh_bvh_probe.json (``--out``).  Every workload is one STEP: a child process of its own under its own
time limit, so a step that hangs or faults ends alone; the parent never opens the device, and after a step that failed it starts no
other.  Method (per step), that of tools/point_mesh_probe.py: ``--warmup`` calls of everything first; a window is as many back-to-back
calls as fill ``--window-ms`` (3 to 2000, sized from a first window of 3) between two device events, ended by a synchronise; the
windows of the variants ALTERNATE, ``--windows`` of each, and the median and the spread (min, max) of the per-call time are recorded.
Nothing here is asserted by a test.

    python3 tools/mesh_bvh_probe.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

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

    def window(fn, calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / calls

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
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    calls = {who: int(min(2000, max(3, args.window_ms / max(window(fn, 3), 1e-6)))) for who, fn in variants.items()}
    times = {who: [] for who in variants}
    for _ in range(args.windows):
        for who, fn in variants.items():
            times[who].append(window(fn, calls[who]))
    row = dict(workload=name, points=P, faces=F, verts=int(verts.shape[0]), leaf_size=int(engine._lib.BVH_LEAF), calls=calls)
    for who, ts in times.items():
        row[f"{who}_ms"] = statistics.median(ts)
        row[f"{who}_ms_min"], row[f"{who}_ms_max"] = min(ts), max(ts)
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
    print("ROW " + json.dumps(row), flush=True)
    print("DEVICE " + json.dumps([torch.cuda.get_device_name(0), engine._lib.load().smil_version().decode()]), flush=True)


if args.step:
    run_step(args.step)
    sys.exit(0)

rows, failed, device = [], [], None
for step in STEPS:
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--window-ms", str(args.window_ms), "--windows", str(args.windows),
           "--warmup", str(args.warmup), "--grid", str(args.grid)]
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
        status, out = done.returncode, done.stdout
        if status != 0:
            sys.stderr.write(done.stderr[-2000:])
    except subprocess.TimeoutExpired:
        status, out = "time limit", ""
    if status != 0:
        failed.append(dict(step=step, status=status))
        print(f"{step}: failed ({status}); no further step is started", flush=True)
        break
    for line in out.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
        elif line.startswith("DEVICE "):
            device = json.loads(line[7:])

result = dict(device=device and device[0], library=device and device[1], dtype="float32",
              baseline="mesh3d.closest_points (the brute force of csrc/point_mesh.hip) in the same run, alternating windows",
              window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, grid=args.grid, failed=failed,
              not_measured=STEPS[len(rows):], rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(f"wrote {args.out}")
sys.exit(1 if failed else 0)
