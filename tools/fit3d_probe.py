"""Timing probe of the 3-D registration path: Stage.step per iteration, the chamfer kernels alone against their
fp32 VALU floor, and the same losses composed from plain torch ops at equal inputs.  Prints one JSON line and writes it to
``--out`` (default profiles/fit3d_probe.json).

With ``--sdf`` it measures the SDF-guided term instead (10 000 vertex samples a side, K = 50) and writes
profiles/fit3d_sdf_probe.json: the ``sdf_distance`` call with gradients, Stage.step with the term on and off, the same term from
plain torch ops (cdist + topk + gathers + softmax under autograd, in chunks of at most 8 meshes to bound its (n, 10 000, 10 000)
matrices), the VALU floor of the two searches and the measured list insertions per query.

Setup: the STICK and mouse models as sources, the Atta worker scan (tests/golden/atta_worker_mesh.npz) as every target, each copy
under its own random rigid motion, B in {1, 16, 64}.  Device events after a warm-up.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from smilify_amd import engine, fit3d  # noqa: E402
from smilify_amd.mesh3d import Meshes  # noqa: E402

MODELS = {"stick": "data/models/SMILy_STICK.npz", "mouse": "data/models/SMILy_Mouse_static_joints.npz"}
VALU_FP32_FLOPS = 157.3e12   # MI355X_MICROARCH: peak fp32 vector rate
FLOPS_PER_PAIR = 8           # 3 sub, 3 mul, 2 add


def rot(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    q = q / q.norm()
    w, x, y, z = q.tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def targets(B, dev):
    d = np.load(os.path.join(REPO, "tests", "golden", "atta_worker_mesh.npz"))
    v = torch.from_numpy(d["verts"]).double()
    v = (v - v.mean(0)) / (v - v.mean(0)).abs().max()
    f = torch.from_numpy(d["faces"].astype(np.int64)).to(dev)
    g = torch.Generator().manual_seed(0)
    vs = [(v @ rot(g).T + 0.1 * torch.randn(3, generator=g, dtype=torch.float64)).float().to(dev) for _ in range(B)]
    return Meshes(vs, [f] * B)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_losses(x, verts, topo, faces):
    """The same losses from plain torch ops (cdist + min, index gathers): the yardstick."""
    d = torch.cdist(x, verts) ** 2
    ch = d.min(2)[0].mean(1).mean() + d.min(1)[0].mean(1).mean()
    e = topo["edges"]
    edge = ((verts[:, e[:, 0]] - verts[:, e[:, 1]]) ** 2).sum(-1).mean()
    p = topo["pairs"]
    v0, v1, a, b = (verts[:, p[:, k]] for k in range(4))
    n0 = torch.cross(v1 - v0, a - v0, dim=-1)
    n1 = -torch.cross(v1 - v0, b - v0, dim=-1)
    normal = (1 - torch.cosine_similarity(n0, n1, dim=-1)).mean()
    s = torch.zeros_like(verts).index_add_(1, topo["rows"], verts[:, topo["cols"]])
    lap = (s * topo["inv_deg"][None, :, None] - verts).norm(dim=-1).mean()
    return ch + edge + 0.01 * normal + 0.1 * lap


SDF_SAMPLES, SDF_K, TORCH_CHUNK = 10000, 50, 8


def torch_sdf(x, y, xs, ys, K):
    """The term from plain torch ops: the yardstick."""
    def z(s):
        return (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True).clamp(min=1e-8)

    def one(q, c, zq, zc):
        d, i = (torch.cdist(q, c) ** 2).topk(K, dim=2, largest=False)
        w = torch.softmax(-(zq[:, :, None] - torch.gather(zc, 1, i.reshape(i.shape[0], -1)).reshape(i.shape)).abs() / 0.1, dim=-1)
        return (w * d).sum(-1).mean(1).sum()

    zx, zy = z(xs), z(ys)
    return (one(x, y, zx, zy) + one(y, x, zy, zx)) / x.shape[0]


def sdf_rows(args, dev):
    rows = []
    for key, path in MODELS.items():
        for B in [int(b) for b in args.batches.split(",")]:
            tgt = targets(B, dev)
            model = fit3d.SMAL3DFitter(batch_size=B, device=dev, model_path=os.path.join(REPO, path))
            with torch.no_grad():
                src = model()[0]
            src_val = (src - src.mean(0)).norm(dim=1)
            tv = tgt.verts_list()[0]
            tgt_val = (tv - tv.mean(0)).norm(dim=1)
            step_ms = {}
            for name, kw in (("off", {}), ("on", dict(sdf_values=tgt_val, source_sdf_values=src_val))):
                stage = fit3d.Stage(args.iters, "all", model, tgt, lr=1e-4, **kw)
                for _ in range(3):
                    stage.optimizer.zero_grad()
                    stage.step(0)
                step_ms[name] = timed(lambda: (stage.optimizer.zero_grad(), stage.step(0)), args.iters)
            with torch.no_grad():
                x, xs, _ = fit3d.sample_vertices_with_index(stage.src_mesh, src_val, SDF_SAMPLES, seed=1)
                y, ys, _ = fit3d.sample_vertices_with_index(tgt, tgt_val, SDF_SAMPLES, seed=2)
            call = lambda: engine.sdf_distance(x, y, xs, ys, SDF_K)  # noqa: E731
            for _ in range(3):
                ins = call()[4]
            call_ms = timed(call, args.iters)
            pairs = 2.0 * B * SDF_SAMPLES * SDF_SAMPLES
            floor_ms = pairs * FLOPS_PER_PAIR / VALU_FP32_FLOPS * 1e3

            def torch_fn():
                for b0 in range(0, B, TORCH_CHUNK):
                    xa = x[b0:b0 + TORCH_CHUNK].clone().requires_grad_(True)
                    ya = y[b0:b0 + TORCH_CHUNK].clone().requires_grad_(True)
                    torch.autograd.grad(torch_sdf(xa, ya, xs[b0:b0 + TORCH_CHUNK], ys[b0:b0 + TORCH_CHUNK], SDF_K), (xa, ya))

            torch_fn()
            torch_ms = timed(torch_fn, 3)
            rows.append(dict(model=key, B=B, V=int(src.shape[0]), samples=SDF_SAMPLES, K=SDF_K, sdf_call_ms=call_ms, sdf_torch_ms=torch_ms,
                             stage_step_sdf_on_ms=step_ms["on"], stage_step_sdf_off_ms=step_ms["off"], search_pairs=pairs,
                             search_valu_floor_ms=floor_ms, search_floor_over_call=floor_ms / call_ms,
                             insertions_per_query=float(ins.item()) / (2.0 * B * SDF_SAMPLES)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sdf", action="store_true", help="measure the SDF-guided term (profiles/fit3d_sdf_probe.json)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "fit3d_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.sdf:
        out = args.out if args.out != ap.get_default("out") else os.path.join(REPO, "profiles", "fit3d_sdf_probe.json")
        res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, torch_chunk_meshes=TORCH_CHUNK, rows=sdf_rows(args, dev))
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res))
        return
    rows = []
    for key, path in MODELS.items():
        for B in [int(b) for b in args.batches.split(",")]:
            tgt = targets(B, dev)
            model = fit3d.SMAL3DFitter(batch_size=B, device=dev, model_path=os.path.join(REPO, path))
            stage = fit3d.Stage(args.iters, "all", model, tgt, lr=1e-4)
            for _ in range(3):
                stage.optimizer.zero_grad()
                stage.step(0)
            step_ms = timed(lambda: (stage.optimizer.zero_grad(), stage.step(0)), args.iters)
            x = stage.last_target_samples.contiguous()
            verts = model().detach().contiguous()
            V = verts.shape[1]
            for _ in range(3):
                engine.chamfer(x, verts)
            ch_ms = timed(lambda: engine.chamfer(x, verts), args.iters)
            pairs = 2.0 * B * x.shape[1] * V
            floor_ms = pairs * FLOPS_PER_PAIR / VALU_FP32_FLOPS * 1e3
            T = stage.src_mesh.topology()
            tt = dict(edges=torch.from_numpy(T.edges).to(dev), pairs=torch.from_numpy(T.pairs).to(dev),
                      rows=torch.from_numpy(np.concatenate([T.edges[:, 0], T.edges[:, 1]])).to(dev),
                      cols=torch.from_numpy(np.concatenate([T.edges[:, 1], T.edges[:, 0]])).to(dev),
                      inv_deg=torch.from_numpy(T.inv_deg.astype(np.float32)).to(dev))
            vg = verts.clone().requires_grad_(True)
            torch_fn = lambda: torch.autograd.grad(torch_losses(x, vg, tt, None), vg)  # noqa: E731
            for _ in range(2):
                torch_fn()
            torch_ms = timed(torch_fn, max(3, args.iters // 4))
            m = Meshes(vg, stage.faces)
            ours_fn = lambda: torch.autograd.grad(fit3d.chamfer_distance(x, vg)[0] + (fit3d.mesh_regularisers(m) * torch.tensor(  # noqa: E731
                [1.0, 0.01, 0.1], device=dev)).sum(), vg)
            for _ in range(2):
                ours_fn()
            ours_ms = timed(ours_fn, args.iters)
            rows.append(dict(model=key, B=B, V=V, samples=int(x.shape[1]), stage_step_ms=step_ms, chamfer_ms=ch_ms,
                             chamfer_pairs=pairs, chamfer_valu_floor_ms=floor_ms, chamfer_frac_of_floor=floor_ms / ch_ms,
                             losses_hip_ms=ours_ms, losses_torch_ms=torch_ms))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
