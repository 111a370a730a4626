"""Times the triangulation kernel (csrc/triangulate.hip) on the GPU against the only alternative the library had before it: the
same algorithm from batched ``torch.linalg.svd`` in float64 on the same GPU.  Device events around each call.

    python tools/triangulate_probe.py [--sizes 3400 340000 3400000] [--cameras 6 18] [--out profiles/triangulate_probe.json]

Per size N Kp, camera count C and method (pair RANSAC, plain DLT): the kernel's time (median of ``--iters`` calls after a warm-up), the
yardstick's (median of ``--yardstick-iters``; it runs in chunks of ``--chunk`` problems because its hypothesis systems alone take
6.4 KB a problem) and their ratio.  A yardstick run that would exceed ``--yardstick-budget`` seconds is timed on as many chunks as fit
and scaled to the full size; the row says so (``yardstick_chunks_timed`` < ``yardstick_chunks``).  The reference's CPU loop (numpy,
one problem at a time) is timed once on 100 problems for scale.  No GPU: the probe fails.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilify_amd import _lib, engine, triangulate  # noqa: E402


def rig(C, rng):
    P = []
    for c in range(C):
        az = 2 * np.pi * c / C + rng.uniform(-0.05, 0.05)
        eye = np.array([4 * np.cos(az), 4 * np.sin(az), 1.5 + 0.5 * (c % 3)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        K = np.array([[1100.0, 0, 640], [0, 1110.0, 512], [0, 0, 1]])
        P.append(K @ np.hstack([R, (-R @ eye)[:, None]]))
    return np.stack(P)


def observations(P, NP, rng, dev):
    """(NP, 1, C, 2) on the device: seeded points, 1 px noise, one view in eight a gross outlier."""
    g = torch.Generator(device=dev).manual_seed(int(rng.integers(1 << 30)))
    Pt = torch.from_numpy(P).to(dev)
    X = torch.rand(NP, 3, device=dev, dtype=torch.float64, generator=g) - 0.5
    h = torch.einsum("cij,nj->nci", Pt, torch.cat([X, torch.ones(NP, 1, device=dev, dtype=torch.float64)], 1))
    obs = h[..., :2] / h[..., 2:3] + torch.randn(NP, len(P), 2, device=dev, dtype=torch.float64, generator=g)
    out = torch.rand(NP, len(P), 1, device=dev, dtype=torch.float64, generator=g) < 0.125
    obs = obs + out * (150.0 + 200.0 * torch.rand(NP, len(P), 2, device=dev, dtype=torch.float64, generator=g))
    return obs[:, None].contiguous()


def torch_dlt(A):
    X = torch.linalg.svd(A)[2][..., -1, :]
    return X[..., :3] / X[..., 3:4]


def torch_errors(Pt, X, obs):
    """X (..., 3), obs (NP, C, 2) -> (..., C)"""
    h = torch.einsum("cij,n...j->n...ci", Pt[:, :, :3], X) + Pt[:, :, 3]
    return torch.linalg.norm(h[..., :2] / h[..., 2:3] - obs.reshape(obs.shape[:1] + (1,) * (X.dim() - 2) + obs.shape[1:]), dim=-1)


def yardstick_chunk(Pt, obs, pairs, thr, min_views, use_ransac):
    """The algorithm of the kernel from batched torch ops, every view valid: obs (n, C, 2) -> (n, 3)."""
    rows = torch.stack([obs[..., 0:1] * Pt[None, :, 2] - Pt[None, :, 0], obs[..., 1:2] * Pt[None, :, 2] - Pt[None, :, 1]], dim=2)  # (n, C, 2, 4)
    n, C = obs.shape[:2]
    keep = torch.ones(n, C, device=obs.device, dtype=torch.bool)
    if use_ransac and C >= 3:
        A = torch.cat([rows[:, pairs[:, 0]], rows[:, pairs[:, 1]]], dim=2)  # (n, H, 4, 4)
        inl = torch_errors(Pt, torch_dlt(A), obs) < thr  # (n, H, C)
        count = inl.sum(-1)
        key = count * 64 + (63 - torch.arange(len(pairs), device=obs.device))
        win = 63 - key.max(dim=1).values % 64
        keep = inl[torch.arange(n, device=obs.device), win]
    X = torch_dlt((rows * keep[:, :, None, None]).reshape(n, 2 * C, 4))
    return torch.where((keep.sum(1) >= min_views)[:, None], X, torch.full_like(X, float("nan")))


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def cpu_loop(P, obs, pairs, thr):
    t0 = time.perf_counter()
    for o in obs:
        rows = np.stack([o[:, 0:1] * P[:, 2] - P[:, 0], o[:, 1:2] * P[:, 2] - P[:, 1]], axis=1)
        best, mask = 0, None
        for i, j in pairs:
            X = np.linalg.svd(np.concatenate([rows[i], rows[j]]))[2][-1]
            h = P @ np.append(X[:3] / X[3], 1.0)
            m = np.linalg.norm(h[:, :2] / h[:, 2:3] - o, axis=1) < thr
            if m.sum() > best:
                best, mask = m.sum(), m
        if mask is not None:
            np.linalg.svd(rows[mask].reshape(-1, 4))
    return (time.perf_counter() - t0) / len(obs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[3400, 340000, 3400000])
    ap.add_argument("--cameras", type=int, nargs="+", default=[6, 18])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--yardstick-iters", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=34000)
    ap.add_argument("--yardstick-budget", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = engine.require_gpu("cuda:0")
    rng = np.random.default_rng(0)
    table = torch.from_numpy(triangulate.pair_table().copy()).to(dev)
    rows = []
    for C in a.cameras:
        P = rig(C, rng)
        Pt = torch.from_numpy(P).to(dev)
        pairs = table[C, :min(C * (C - 1) // 2, _lib.TRI_MAX_HYP)].long()
        for NP in a.sizes:
            obs = observations(P, NP, rng, dev)
            for use_ransac in (True, False):
                mode = _lib.TRI_RANSAC if use_ransac else 0
                run = lambda: engine.triangulate(Pt, obs, None, table, min_views=2, reproj_threshold=15.0, mode=mode)  # noqa: E731
                xyz = run()[0]
                k = timed(run, a.iters)
                chunks = [obs[s:s + a.chunk, 0] for s in range(0, NP, a.chunk)]
                ref = yardstick_chunk(Pt, chunks[0], pairs, 15.0, 2, use_ransac)  # warm-up, and the same points
                torch.cuda.synchronize()
                agree = float(((xyz[:len(ref), 0] - ref).abs().amax(1) <= 1e-6 * ref.abs().amax(1)).double().mean())
                t0 = time.perf_counter()
                one = timed(lambda: yardstick_chunk(Pt, chunks[0], pairs, 15.0, 2, use_ransac), 1)[0]
                fit = max(1, min(len(chunks), int(a.yardstick_budget * 1e3 / a.yardstick_iters / max(one, 1e-3))))
                y = [t * len(chunks) / fit for t in timed(lambda: [yardstick_chunk(Pt, c, pairs, 15.0, 2, use_ransac) for c in chunks[:fit]],
                                                          a.yardstick_iters)]
                row = dict(problems=NP, cameras=C, method="ransac" if use_ransac else "dlt", kernel_ms_median=k[len(k) // 2], kernel_ms_min=k[0],
                           kernel_ms_max=k[-1], yardstick_ms_median=y[len(y) // 2], yardstick_ms_min=y[0], yardstick_chunks=len(chunks),
                           yardstick_chunks_timed=fit, speedup=y[len(y) // 2] / k[len(k) // 2], points_agreeing=agree,
                           wall_s=time.perf_counter() - t0)
                rows.append(row)
                print(json.dumps(row), flush=True)
    # the reference's loop, once, for scale: the last rig, its first 100 problems
    cpu = cpu_loop(P, obs[:100, 0].cpu().numpy(), pairs.cpu().numpy(), 15.0)
    print(json.dumps(dict(cpu_loop_s_per_problem=cpu, cameras=a.cameras[-1])), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, yardstick_iters=a.yardstick_iters, chunk=a.chunk,
                  yardstick_budget=a.yardstick_budget, rows=rows,
                  cpu_loop_s_per_problem=cpu, cpu_loop_cameras=a.cameras[-1])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(done=True, rows=len(rows))))


if __name__ == "__main__":
    main()
