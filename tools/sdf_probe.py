"""Timing probe of the spatial-diameter ray cast: all-faces ``compute_sdf`` with 30 rays on the STICK
template, the Atta worker scan (tests/golden/atta_worker_mesh.npz) and the mouse template.  Prints one JSON line and writes it to
``--out`` (default profiles/sdf_ray_probe.json).

Per mesh: ``smil_ray_diameters`` alone on resident inputs (device events after a warm-up, ``--iters`` calls), the whole
``compute_sdf`` (host clock around a call that ends in a synchronise: it draws F x 30 directions on the CPU and uploads them), the
fp32 VALU floor of the F x 30 x F ray-face tests at the 46 operations the kernel issues per test, and the reference's vectorised
formula from plain torch ops on the same GPU, batched over rays and chunked (``torch_cast``).

The cast kernel's own time comes from a separate run under the profiler, one mesh per run::

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o stick -- python3 tools/sdf_probe.py --trace stick

and is folded in with ``--kernel-stats stick=DIR/..._kernel_stats.csv,atta=...``.  ``--reference-seconds`` records the reference's own
``compute_sdf`` on the fixture mesh of tests/golden (320 faces, 30 rays), timed on a CPU by tests/golden/make_sdf_ray_fixture.py.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from smilify_amd import engine, sdf  # noqa: E402
from smilify_amd.mesh3d import Meshes  # noqa: E402
from smilify_amd.model_io import load_model  # noqa: E402

MODELS = {"stick": "data/models/SMILy_STICK.npz", "mouse": "data/models/SMILy_Mouse_static_joints.npz"}
VALU_FP32_FLOPS = 157.3e12  # MI355X_MICROARCH: peak fp32 vector rate
FLOPS_PER_TEST = 46         # k_ray_cast as written: s 3, h 9, a 5, s.h 5, q 9, d.q 5, e2.q 5, 1/a 1, u v t 3, u + v 1
NUM_RAYS = 30


def load(name):
    if name == "atta":
        d = np.load(os.path.join(REPO, "tests", "golden", "atta_worker_mesh.npz"))
        return torch.from_numpy(d["verts"].astype(np.float32)), torch.from_numpy(d["faces"].astype(np.int64))
    t = load_model(os.path.join(REPO, MODELS[name]))
    return torch.from_numpy(np.asarray(t.v_template, np.float32)), torch.from_numpy(np.asarray(t.faces, np.int64))


def inputs(v, f, dev, seed=0):
    """The device inputs of the all-faces cast, formed as compute_sdf forms them."""
    torch.manual_seed(seed)
    fv = v[f]
    n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    diag = torch.norm(v.max(0)[0] - v.min(0)[0])
    dirs = torch.cat([sdf.generate_random_directions_batch(n[s:s + sdf.BATCH], NUM_RAYS) for s in range(0, len(f), sdf.BATCH)])
    origins = fv.mean(1) + n * (diag * 0.0001)
    return dict(verts=v.to(dev), faces=f.to(torch.int32).to(dev), origins=origins.to(dev), own=torch.arange(len(f), dtype=torch.int32).to(dev),
                dirs=dirs.to(dev), t_min=float(diag * 0.0001), d_lo=float(diag * 0.001), d_hi=float(diag * 0.2), cap=max(len(f) // 2, 1))


def cast(x, want_ray_t=False):
    return engine.ray_diameters(x["verts"], x["faces"], x["origins"], x["own"], x["dirs"], x["t_min"], x["d_lo"], x["d_hi"], x["cap"],
                                want_ray_t=want_ray_t)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_cast(x, budget=1 << 24):
    """The largest hit of every ray from the reference's formula (SDF_tests.py:146-213) in plain torch ops, ``budget`` ray-face
    pairs at a time: (S, R) with -1 where nothing is hit."""
    v, f = x["verts"], x["faces"].long()
    v0 = v[f[:, 0]]
    e1, e2 = v[f[:, 1]] - v0, v[f[:, 2]] - v0
    S, Rn, F = x["dirs"].shape[0], x["dirs"].shape[1], len(f)
    o = x["origins"].repeat_interleave(Rn, 0)
    own = x["own"].long().repeat_interleave(Rn, 0)
    d = x["dirs"].reshape(-1, 3)
    out = torch.empty(S * Rn, device=v.device)
    step = max(1, budget // F)
    fid = torch.arange(F, device=v.device)
    for r0 in range(0, S * Rn, step):
        dd = d[r0:r0 + step, None, :]
        h = torch.cross(dd.expand(-1, F, -1), e2[None].expand(dd.shape[0], -1, -1), dim=2)
        a = (e1[None] * h).sum(2)
        fi = 1.0 / a
        s = o[r0:r0 + step, None, :] - v0[None]
        u = fi * (s * h).sum(2)
        q = torch.cross(s, e1[None].expand_as(s), dim=2)
        vv = fi * (dd * q).sum(2)
        t = fi * (e2[None] * q).sum(2)
        hit = (fid[None] != own[r0:r0 + step, None]) & (a.abs() > 1e-6) & (u >= 0) & (u <= 1) & (vv >= 0) & (u + vv <= 1) & (t > x["t_min"])
        out[r0:r0 + step] = torch.where(hit, t, torch.full_like(t, -1.0)).max(1)[0]
    return out.reshape(S, Rn)


def kernel_stats(spec):
    """{mesh: average k_ray_cast duration in ms} from 'mesh=stats.csv,...'."""
    out = {}
    for item in filter(None, (spec or "").split(",")):
        name, path = item.split("=", 1)
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if row["Name"].startswith("k_ray_cast"):
                    out[name] = dict(cast_kernel_ms=float(row["AverageNs"]) / 1e6, calls=int(row["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--meshes", type=str, default="stick,atta,mouse")
    ap.add_argument("--trace", type=str, default=None, help="only run the cast of this mesh a few times (for a profiler run)")
    ap.add_argument("--kernel-stats", type=str, default=None)
    ap.add_argument("--reference-seconds", type=float, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "sdf_ray_probe.json"))
    args = ap.parse_args()
    dev = engine.require_gpu("cuda:0")
    if args.trace:
        x = inputs(*load(args.trace), dev)
        for _ in range(6):
            cast(x)
        torch.cuda.synchronize()
        return
    stats = kernel_stats(args.kernel_stats)
    rows = []
    for name in args.meshes.split(","):
        v, f = load(name)
        x = inputs(v, f, dev)
        F = len(f)
        tests = F * NUM_RAYS * F
        for _ in range(3):
            cast(x)
        call_ms = timed(lambda: cast(x), args.iters)
        mesh = Meshes(verts=[v.to(dev)], faces=[f.to(dev)])
        sdf.compute_sdf(mesh, num_samples=-1, num_rays=NUM_RAYS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            sdf.compute_sdf(mesh, num_samples=-1, num_rays=NUM_RAYS)
        torch.cuda.synchronize()
        whole_ms = (time.perf_counter() - t0) / 3 * 1e3
        want = torch_cast(x)
        torch_ms = timed(lambda: torch_cast(x), 2)
        got = cast(x, want_ray_t=True)[1]
        same = ((got >= 0) == (want >= 0)).float().mean().item()
        floor_ms = tests * FLOPS_PER_TEST / VALU_FP32_FLOPS * 1e3
        row = dict(mesh=name, V=len(v), F=F, rays=F * NUM_RAYS, tests=tests, ray_diameters_ms=call_ms, compute_sdf_ms=whole_ms,
                   torch_cast_ms=torch_ms, torch_over_hip=torch_ms / call_ms, valu_floor_ms=floor_ms, share_of_floor_call=floor_ms / call_ms,
                   hit_decisions_equal_to_torch=same)
        if name in stats:
            row.update(stats[name], share_of_floor_kernel=floor_ms / stats[name]["cast_kernel_ms"],
                       tests_per_second=tests / (stats[name]["cast_kernel_ms"] * 1e-3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), num_rays=NUM_RAYS, iters=args.iters, flops_per_test=FLOPS_PER_TEST,
               valu_fp32_flops=VALU_FP32_FLOPS, rows=rows)
    if args.reference_seconds is not None:
        res["reference_compute_sdf_fixture_cpu_s"] = args.reference_seconds
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
