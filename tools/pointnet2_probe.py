"""Timing probe of the PointNet++ set-abstraction kernels: farthest point sampling, the ball query at three
radii and the grouping (forward, and backward where there are features) at the shapes of the regressor's two multi-scale layers -
512 centres, radii 0.1 / 0.2 / 0.4, nsample 16 / 32 / 128, no features; 128 centres from 512 points, radii 0.2 / 0.4 / 0.8, nsample
32 / 64 / 128, 320 features - and the two layers' forward together, for B in {1, 16, 64} and clouds of 3 000 and 5 000 points drawn
from the Atta scan (tests/golden/atta_worker_mesh.npz).

The yardstick is the reference's algorithm from plain torch ops on the same GPU and inputs, restated here: the npoint-iteration
loop, the sort of the (B, S, N) index tensor per radius, and index gathers + cat + permute(...).contiguous().  Every operation must
beat its yardstick by more than the 8 % this project has seen between two measurements of one configuration (DESIGN.md section
4.4); the exit status is 1 otherwise.  Device events after a warm-up.  Prints one JSON line per row and writes ``--out``.

The FPS floor is a latency chain, not a bandwidth figure: npoint x (the distance update and argmax over the thread's points + two
key reductions + one barrier and one LDS round trip), from the issue costs of MI355X (2 cycles per wave64 VALU instruction and SIMD,
so 2 x waves-per-SIMD cycles per instruction of the workgroup; 4 when one wave runs alone) at 2.4 GHz.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from smilify_amd import engine, pointnet2  # noqa: E402

LAYER1 = dict(npoint=512, radii=[0.1, 0.2, 0.4], nsample=[16, 32, 128], D=0, mlp=[[32, 32, 64], [64, 64, 128], [64, 96, 128]])
LAYER2 = dict(npoint=128, radii=[0.2, 0.4, 0.8], nsample=[32, 64, 128], D=320, mlp=[[64, 64, 128], [128, 128, 256], [128, 128, 256]])
MARGIN = 1.08
CLOCK_HZ = 2.4e9
VALU_PER_POINT, VALU_PER_REDUCTION, HOP_CYCLES = 15, 45, 164  # update + argmax; four DPP steps on two words + read-lanes; barrier + LDS write/read


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def clouds(B, N, dev):
    v = np.load(os.path.join(REPO, "tests", "golden", "atta_worker_mesh.npz"))["verts"]
    rng = np.random.default_rng(B * 100003 + N)
    return torch.from_numpy(np.stack([pointnet2.pc_normalize(v[rng.permutation(len(v))[:N]]) for _ in range(B)]).astype(np.float32)).to(dev)


# ---- the yardstick: the reference's algorithm from plain torch ops ------------------------------------------------------------------
def torch_fps(xyz, npoint, start):
    B, N, _ = xyz.shape
    out = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    dist = torch.full((B, N), 1e10, device=xyz.device)
    far, rows = start.clone(), torch.arange(B, device=xyz.device)
    for i in range(npoint):
        out[:, i] = far
        d = ((xyz - xyz[rows, far].view(B, 1, 3)) ** 2).sum(-1)
        closer = d < dist
        dist[closer] = d[closer]
        far = dist.max(-1)[1]
    return out


def torch_ball(radius, nsample, xyz, q):
    B, N, _ = xyz.shape
    S = q.shape[1]
    idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    idx[pointnet2.square_distance(q, xyz) > radius ** 2] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, idx.shape[2])
    return torch.where(idx == N, first, idx)


def torch_group(xyz, centres, feats, idx):
    rows = torch.arange(idx.shape[0], device=idx.device)[:, None, None]
    g = xyz[rows, idx] - centres[:, :, None, :]
    if feats is not None:
        g = torch.cat([feats[rows, idx], g], -1)
    return g.permute(0, 3, 2, 1).contiguous()


def torch_layer(layer, xyz, feats, start):
    new_xyz = xyz[torch.arange(xyz.shape[0], device=xyz.device)[:, None], torch_fps(xyz, layer.npoint, start)]
    outs = []
    for i, (r, k) in enumerate(zip(layer.radius_list, layer.nsample_list)):
        g = torch_group(xyz, new_xyz, feats, torch_ball(r, k, xyz, new_xyz))
        outs.append(pointnet2._mlp(g, layer.conv_blocks[i], layer.bn_blocks[i]).max(2)[0])
    return new_xyz, torch.cat(outs, 1)


def fps_floor_ms(N, npoint):
    ppt, threads = (4, 64) if N <= 256 else (8, 64) if N <= 512 else (4, 0) if N <= 4096 else (8, 0) if N <= 8192 else (16, 0)
    threads = threads or (((N + ppt - 1) // ppt + 63) // 64) * 64
    waves_per_simd = max(1, threads // 256)
    per_instr = 4 if threads == 64 else 2 * waves_per_simd
    reductions, hop = (1, 0) if threads == 64 else (2, HOP_CYCLES)
    return npoint * (per_instr * (VALU_PER_POINT * ppt + VALU_PER_REDUCTION * reductions) + hop) / CLOCK_HZ * 1e3


def probe_layer(cfg, xyz, feats, iters, slow_iters):
    """One layer's three operations against their yardsticks; returns (row, centres)."""
    B, N, _ = xyz.shape
    S, D = cfg["npoint"], cfg["D"]
    start = torch.zeros(B, dtype=torch.long, device=xyz.device)
    start32 = start.int()
    row = dict(B=B, N=N, S=S, D=D)
    ours = lambda: engine.fps(xyz, S, start32)  # noqa: E731
    fps_idx = ours().long()
    row["fps_rows_equal"] = float((fps_idx == torch_fps(xyz, S, start)).all(-1).float().mean())  # (torch's tie index on a GPU is unspecified)
    row["fps_ms"], row["fps_torch_ms"] = timed(ours, iters), timed(lambda: torch_fps(xyz, S, start), slow_iters)
    row["fps_floor_ms"] = fps_floor_ms(N, S)
    row["fps_floor_share"] = row["fps_floor_ms"] / row["fps_ms"]
    centres = pointnet2.index_points(xyz, fps_idx).contiguous()
    ours = lambda: engine.ball_query(xyz, centres, cfg["radii"], cfg["nsample"])  # noqa: E731
    idx = ours()
    yard = lambda: [torch_ball(r, k, xyz, centres) for r, k in zip(cfg["radii"], cfg["nsample"])]  # noqa: E731
    same = [float((a.long() == b).all(-1).float().mean()) for a, b in zip(idx, yard())]
    row["ball_rows_equal"] = min(same)
    row["ball_ms"], row["ball_torch_ms"] = timed(ours, iters), timed(yard, slow_iters)
    ours = lambda: [engine.group_points(xyz, centres, feats, i, True) for i in idx]  # noqa: E731
    long_idx = [i.long().clamp(max=N - 1) for i in idx]
    yard = lambda: [torch_group(xyz, centres, feats, i) for i in long_idx]  # noqa: E731
    ours(), yard()
    row["group_ms"], row["group_torch_ms"] = timed(ours, iters), timed(yard, slow_iters)
    if D:
        d_out = [torch.randn(B, 3 + D, i.shape[2], S, device=xyz.device) for i in idx]
        ours = lambda: [engine.group_points_backward(g, i, N, D, True, True) for g, i in zip(d_out, idx)]  # noqa: E731
        fg = feats.clone().requires_grad_(True)

        def yard():
            for g, i in zip(d_out, long_idx):
                torch.autograd.grad(torch_group(xyz, centres, fg, i), fg, g)

        ours(), yard()
        row["group_bwd_ms"], row["group_fwd_bwd_torch_ms"] = timed(ours, iters), timed(yard, slow_iters)
    return row, centres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slow-iters", type=int, default=3, help="iterations of the torch yardsticks")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--sizes", type=str, default="3000,5000")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "pointnet2_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sa1 = pointnet2.PointNetSetAbstractionMsg(LAYER1["npoint"], LAYER1["radii"], LAYER1["nsample"], 0, LAYER1["mlp"]).to(dev).eval()
    sa2 = pointnet2.PointNetSetAbstractionMsg(LAYER2["npoint"], LAYER2["radii"], LAYER2["nsample"], 320, LAYER2["mlp"]).to(dev).eval()
    rows, failed = [], []
    for B in [int(b) for b in args.batches.split(",")]:
        for N in [int(n) for n in args.sizes.split(",")]:
            xyz = clouds(B, N, dev)
            r1, centres = probe_layer(LAYER1, xyz, None, args.iters, args.slow_iters)
            feats = torch.randn(B, LAYER1["npoint"], 320, device=dev)
            r2, _ = probe_layer(LAYER2, centres, feats, args.iters, args.slow_iters)
            start = torch.zeros(B, dtype=torch.long, device=dev)

            def ours():
                torch.manual_seed(0)
                x1, f1 = sa1(xyz.transpose(1, 2), None)
                return sa2(x1, f1)

            def yard():
                x1, f1 = torch_layer(sa1, xyz, None, start)
                return torch_layer(sa2, x1, f1.transpose(1, 2), start)

            with torch.no_grad():
                ours(), yard()
                both = dict(B=B, N=N, layers_ms=timed(ours, max(3, args.iters // 4)), layers_torch_ms=timed(yard, args.slow_iters))
            for name, row in (("layer1", r1), ("layer2", r2), ("both", both)):
                row["what"] = name
                for k in [k for k in row if k.endswith("_torch_ms")]:
                    mine = row["group_ms"] + row["group_bwd_ms"] if k == "group_fwd_bwd_torch_ms" else row[k.replace("_torch", "")]
                    row[k.replace("_torch_ms", "_speedup")] = row[k] / mine
                    if not row[k] > MARGIN * mine:
                        failed.append((name, B, N, k))
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, torch_iters=args.slow_iters, margin=MARGIN, failed=failed, rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(dict(failed=failed)))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
