"""Times the point refinement kernel (csrc/refine_points.hip) on the GPU against the same Levenberg-Marquardt from batched float64 torch
ops on the same GPU.  Device events around each call, profiler off.

    python tools/refine_points_probe.py [--sizes 3400 340000 3400000] [--cameras 6 18] [--out profiles/refine_points_probe.json]

Per size N Kp and camera count C: seeded observations (1 px noise, one view in eight a gross outlier), the triangulation kernel's own
pair-RANSAC points, masks and undistorted observations as the start, then the refinement kernel's time (median of ``--iters`` calls
after a warm-up) and the yardstick's.  The yardstick is the LM of include/smilfit.h rule for rule on whole batches; a batch iterates
until its last problem is done, so it runs the kernel's LARGEST trial count of the batch, and the kernel is timed with that count as
its ``max_steps`` (the same results: no problem needs more).  The yardstick runs in chunks of ``--chunk`` problems, median of
``--yardstick-iters``; a run that would exceed ``--yardstick-budget`` seconds is timed on the leading chunks and scaled to the full
size, and the row says so (``yardstick_chunks_timed`` < ``yardstick_chunks``).  For scale the row also carries the yardstick's first
chunk at the kernel's MEAN trial count, scaled to the full size: what a batched LM would cost if it could stop where the average
problem does.  No GPU: the probe fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilify_amd import _lib, engine, triangulate  # noqa: E402
from tools.triangulate_probe import observations, rig, timed  # noqa: E402


def torch_lm(Pt, obs, bits, X0, f_scale, steps):
    """The rules of smil_refine_points on a batch: obs (n, C, 2), bits (n, C) bool, X0 (n, 3) -> (n, 3)."""
    n = len(X0)
    cur, cand = X0.clone(), X0.clone()
    lam = torch.full((n,), 1e-3, device=X0.device, dtype=torch.float64)
    cost_cur = torch.full((n,), float("nan"), device=X0.device, dtype=torch.float64)
    g, H = torch.zeros(n, 3, device=X0.device, dtype=torch.float64), torch.zeros(n, 3, 3, device=X0.device, dtype=torch.float64)
    done = bits.sum(1) < 2
    A3, p3 = Pt[:, :, :3], Pt[:, :, 3]
    for step in range(steps):
        h = torch.einsum("cij,nj->nci", A3, cand) + p3
        q = h[..., :2] / h[..., 2:3]
        f = torch.where(bits[..., None], q - obs, 0.0)
        J = (Pt[None, :, :2, :3] - q[..., None] * Pt[None, :, 2:3, :3]) / h[..., 2, None, None]
        z = (f / f_scale) ** 2
        hh = torch.sqrt(1.0 + z)
        w = torch.where(bits[..., None], 1.0 / hh, 0.0)
        cost = 0.5 * f_scale ** 2 * (2.0 * z / (hh + 1.0)).sum((1, 2))
        finite = torch.isfinite(cost)
        if step == 0:
            done = done | ~finite
            accept = ~done
        else:
            accept = finite & (cost < cost_cur) & ~done
            small = accept & (cost_cur - cost < 1e-12 * cost_cur)
            lam = torch.where(done, lam, torch.where(accept, torch.clamp(lam / 10.0, min=1e-12), lam * 10.0))
            done = done | small
        cur = torch.where(accept[:, None], cand, cur)
        g = torch.where(accept[:, None], torch.einsum("ncki,nck->ni", J, w * f), g)
        H = torch.where(accept[:, None, None], torch.einsum("ncki,nck,nckj->nij", J, w, J), H)
        cost_cur = torch.where(accept, cost, cost_cur)
        done = done | (lam > 1e12)
        A = H + lam[:, None, None] * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(A)
        d = torch.cholesky_solve(-g[:, :, None], L)[:, :, 0]
        ok = (info == 0) & torch.isfinite(d).all(1)
        cand = torch.where((ok & ~done)[:, None], cur + d, cur)
        lam = torch.where(ok | done, lam, lam * 10.0)
        done = done | (lam > 1e12)
    return cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[3400, 340000, 3400000])
    ap.add_argument("--cameras", type=int, nargs="+", default=[6, 18])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--yardstick-iters", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=34000)
    ap.add_argument("--yardstick-budget", type=float, default=15.0)
    ap.add_argument("--f-scale", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = engine.require_gpu("cuda:0")
    rng = np.random.default_rng(0)
    table = torch.from_numpy(triangulate.pair_table().copy()).to(dev)
    rows = []
    for C in a.cameras:
        Pt = torch.from_numpy(rig(C, rng)).to(dev)
        lanes = torch.arange(C, device=dev, dtype=torch.int32)
        for NP in a.sizes:
            obs = observations(Pt.cpu().numpy(), NP, rng, dev)
            tri = engine.triangulate(Pt, obs, None, table, min_views=2, reproj_threshold=15.0, mode=_lib.TRI_RANSAC, want_inlier_mask=True,
                                     want_undistorted=True)
            xyz0, mask, und = tri[0], tri[5], tri[6]
            full = engine.refine_points(Pt, und, mask, xyz0, f_scale=a.f_scale)
            steps = int(full[3].max().item())
            run = lambda: engine.refine_points(Pt, und, mask, xyz0, f_scale=a.f_scale, max_steps=steps)  # noqa: E731
            out = run()
            assert torch.equal(out[0], full[0]) or bool(torch.isnan(out[0]).any())
            k = timed(run, a.iters)
            bits = ((mask[:, 0, None] >> lanes) & 1).bool()
            chunks = [slice(s, min(NP, s + a.chunk)) for s in range(0, NP, a.chunk)]
            one_chunk = lambda s: torch_lm(Pt, und[s, 0], bits[s], xyz0[s, 0], a.f_scale, steps)  # noqa: E731
            ref = one_chunk(chunks[0])  # warm-up, and the same points
            torch.cuda.synchronize()
            good = out[1][chunks[0], 0] <= _lib.REFINE_STEP_LIMIT
            agree = float(((out[0][chunks[0], 0] - ref).abs().amax(1) <= 1e-6 * ref.abs().amax(1))[good].double().mean())
            t0 = time.perf_counter()
            one = timed(lambda: one_chunk(chunks[0]), 1)[0]
            fit = max(1, min(len(chunks), int(a.yardstick_budget * 1e3 / a.yardstick_iters / max(one, 1e-3))))
            y = [t * len(chunks) / fit for t in timed(lambda: [one_chunk(s) for s in chunks[:fit]], a.yardstick_iters)]
            mean_steps = int(np.ceil(float(out[3].double().mean())))  # for scale: the first chunk at the kernel's MEAN trial count
            ym = [t * NP / (chunks[0].stop - chunks[0].start) for t in
                  timed(lambda: torch_lm(Pt, und[chunks[0], 0], bits[chunks[0]], xyz0[chunks[0], 0], a.f_scale, mean_steps), a.yardstick_iters)]
            row = dict(problems=NP, cameras=C, steps=steps, mean_steps=mean_steps, yardstick_at_mean_steps_ms_first_chunk_scaled=ym[len(ym) // 2], mean_trials=float(out[3].double().mean()), refined=int((out[1] <= _lib.REFINE_STEP_LIMIT).sum()),
                       kernel_ms_median=k[len(k) // 2], kernel_ms_min=k[0], kernel_ms_max=k[-1], yardstick_ms_median=y[len(y) // 2],
                       yardstick_ms_min=y[0], yardstick_chunks=len(chunks), yardstick_chunks_timed=fit, speedup=y[len(y) // 2] / k[len(k) // 2],
                       points_agreeing=agree, wall_s=time.perf_counter() - t0)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del obs, tri, xyz0, mask, und, full, out, bits, ref
    result = dict(device=torch.cuda.get_device_name(0), iters=a.iters, yardstick_iters=a.yardstick_iters, chunk=a.chunk,
                  yardstick_budget=a.yardstick_budget, f_scale=a.f_scale, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(done=True, rows=len(rows))))


if __name__ == "__main__":
    main()
