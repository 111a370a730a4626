"""Times the camera refinement (csrc/refine.hip) on the GPU against two baselines: the same Levenberg-Marquardt from batched float64
torch operations on the same GPU (analytic Jacobian, ``torch.linalg.cholesky``, one host read of the accept flags per step, which is
how such a loop is written in torch), and scipy's ``least_squares`` (trf, soft_l1, numerical Jacobian: what the reference runs) on
the host CPU, one camera after the other.

    python tools/refine_probe.py [--out profiles/refine_probe.json] [--scipy-cameras 2]

Two sizes: the test fixture's twelve cameras (19 .. 549 correspondences; the torch baseline needs equal counts and is left out
there) and 12 x 200 000 correspondences (the reference's ``--max_points_per_cam`` default).  Per size: the time of one (accumulate,
step) pair (device events around ``smil_refine_evaluate`` plus one step's worth, median of ``--iters``), and the wall time of one
converged camera set (``optimize_cameras`` without the host-side statistics: ``engine.refine_cameras`` on resident tensors).  scipy
at the large size is timed on ``--scipy-cameras`` cameras and scaled to twelve; the row says so.  No GPU: the probe fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_ref as R  # noqa: E402
from smilify_amd import engine  # noqa: E402


def synthetic(C, M, rng):
    """C perturbed look-at cameras with M correspondences each: (init (C,10), pts_3d (C,M,3), pts_2d (C,M,2))."""
    init, p3, p2 = [], [], []
    for c in range(C):
        az = 2 * np.pi * c / C
        eye = np.array([4 * np.cos(az), 4 * np.sin(az), 1.5 + 0.5 * (c % 3)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        Rm = np.stack([x, np.cross(z, x), z])
        from smilify_amd.refine_cameras import rotation_to_rvec

        true = np.concatenate([rotation_to_rvec(Rm), -Rm @ eye, [1100.0, 1110.0, 640.0, 512.0]])
        X = rng.uniform(-0.5, 0.5, (M, 3))
        proj = R.jacobian(true, X)[0] + rng.normal(0.0, 1.0, (M, 2))
        bad = rng.uniform(size=M) < 0.08
        proj[bad] += rng.uniform(60.0, 300.0, (int(bad.sum()), 2))
        x0 = true + np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.02, 3), rng.uniform(-30, 30, 2), rng.uniform(-8, 8, 2)])
        init.append(x0), p3.append(X), p2.append(proj)
    return np.stack(init), np.stack(p3), np.stack(p2)


def torch_eval(x, p3, p2, fs):
    """cost (C), g (C,10), H (C,10,10) of x (C,10) over p3 (C,M,3), p2 (C,M,2): the restatement's formulas, batched."""
    r = x[:, :3]
    t2 = (r * r).sum(1)
    th = torch.sqrt(t2)
    a, b = torch.sin(th) / th, (1 - torch.cos(th)) / t2
    a1, b1 = (torch.cos(th) - a) / t2, (a - 2 * b) / t2
    gen = torch.from_numpy(R.GEN).to(x.device)
    K = torch.einsum("ck,kij->cij", r, gen)
    K2 = K @ K
    Rm = torch.eye(3, device=x.device, dtype=x.dtype) + a[:, None, None] * K + b[:, None, None] * K2
    dR = (r[:, :, None, None] * (a1[:, None, None] * K + b1[:, None, None] * K2)[:, None] + a[:, None, None, None] * gen
          + b[:, None, None, None] * (gen @ K[:, None] + K[:, None] @ gen))
    Xc = p3 @ Rm.transpose(1, 2) + x[:, None, 3:6]
    iz = 1.0 / Xc[..., 2]
    xn, yn = Xc[..., 0] * iz, Xc[..., 1] * iz
    fx, fy = x[:, 6:7], x[:, 7:8]
    zero = torch.zeros_like(iz)
    du, dv = torch.stack([fx * iz, zero, -fx * xn * iz], -1), torch.stack([zero, fy * iz, -fy * yn * iz], -1)
    D = torch.einsum("ckij,cmj->cmki", dR, p3)
    one = torch.ones_like(iz)
    Ju = torch.cat([torch.einsum("cmi,cmki->cmk", du, D), du, torch.stack([xn, zero, one, zero], -1)], -1)
    Jv = torch.cat([torch.einsum("cmi,cmki->cmk", dv, D), dv, torch.stack([zero, yn, zero, one], -1)], -1)
    f = torch.stack([fx * xn + x[:, 8:9], fy * yn + x[:, 9:10]], -1) - p2
    h = torch.sqrt(1 + (f / fs) ** 2)
    w = 1 / h
    cost = 0.5 * fs * fs * (2 * (h - 1)).sum((1, 2))
    g = torch.einsum("cmk,cm->ck", Ju, w[..., 0] * f[..., 0]) + torch.einsum("cmk,cm->ck", Jv, w[..., 1] * f[..., 1])
    H = torch.einsum("cmk,cml->ckl", Ju * w[..., 0:1], Ju) + torch.einsum("cmk,cml->ckl", Jv * w[..., 1:2], Jv)
    return cost, g, H


def torch_lm(x0, p3, p2, fs=5.0, max_steps=100):
    """The kernel's rules on batched tensors; returns (x, steps)."""
    cur, cand = x0.clone(), x0.clone()
    C = len(x0)
    lam = torch.full((C,), 1e-3, device=x0.device, dtype=x0.dtype)
    done = torch.zeros(C, dtype=torch.bool, device=x0.device)
    cost_cur = g = H = None
    for step in range(max_steps):
        cost_new, g_new, H_new = torch_eval(cand, p3, p2, fs)
        if step == 0:
            cost_cur, g, H = cost_new, g_new, H_new
        else:
            acc = torch.isfinite(cost_new) & (cost_new < cost_cur) & ~done
            rej = ~acc & ~done
            small = acc & (cost_cur - cost_new < 1e-12 * cost_cur)
            cur = torch.where(acc[:, None], cand, cur)
            g, H = torch.where(acc[:, None], g_new, g), torch.where(acc[:, None, None], H_new, H)
            cost_cur = torch.where(acc, cost_new, cost_cur)
            lam = torch.where(acc, torch.clamp(lam / 10, min=1e-12), torch.where(rej, lam * 10, lam))
            done = done | small | (lam > 1e12)
        if bool(done.all()):  # the host read of a torch loop
            return cur, step + 1
        A = H + lam[:, None, None] * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(A)
        d = torch.cholesky_solve(-g[:, :, None], L)[:, :, 0]
        ok = (info == 0) & torch.isfinite(d).all(1)
        cand = torch.where((ok & ~done)[:, None], cur + d, cur)
        lam = torch.where(~ok & ~done, lam * 10, lam)
    return cur, max_steps


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts)), out


def scipy_set(init, cors, cameras):
    from scipy.optimize import least_squares

    from smilify_amd import refine_cameras as rc

    t, nfev = time.perf_counter(), []
    for c in cameras:
        cam = R.camera_of(init[c])
        res = least_squares(rc.reprojection_residuals, init[c], args=(cors[c][0], cors[c][1], cam, True), method="trf", loss="soft_l1",
                            f_scale=5.0, max_nfev=500)
        nfev.append(int(res.nfev))
    return 1e3 * (time.perf_counter() - t), nfev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_probe.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--set-iters", type=int, default=5)
    ap.add_argument("--scipy-cameras", type=int, default=2)
    ap.add_argument("--large", type=int, default=200000)
    args = ap.parse_args()
    dev = engine.require_gpu("cuda:0")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev)  # noqa: E731
    rows = []

    fx = R.fixture()
    cors = R.correspondences(fx)
    sizes = [("fixture", fx["init_params"], cors, None)]
    init, p3, p2 = synthetic(12, args.large, np.random.default_rng(5))
    sizes.append((f"12x{args.large}", init, [(p3[c], p2[c]) for c in range(12)], (p3, p2)))
    for label, init, cors, dense in sizes:
        offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cors])]).astype(np.int64)
        P3, P2, X0 = up(np.concatenate([c[0] for c in cors])), up(np.concatenate([c[1] for c in cors])), up(init)
        row = dict(size=label, cameras=len(cors), correspondences=int(offsets[-1]), device=torch.cuda.get_device_name(0))
        row["kernel_accumulate_ms"] = timed(lambda: engine.refine_evaluate(P3, P2, offsets, X0), args.iters)
        for steps in (2, 3):  # the difference of two bounded runs: one (accumulate, step) pair without the call's fixed cost
            row[f"kernel_{steps}_pairs_ms"] = timed(lambda: engine.refine_cameras(P3, P2, offsets, X0, max_steps=steps), args.iters)
        row["kernel_pair_ms"] = row["kernel_3_pairs_ms"] - row["kernel_2_pairs_ms"]
        ms, out = wall(lambda: engine.refine_cameras(P3, P2, offsets, X0), args.set_iters)
        row["kernel_set_ms"], row["kernel_set_pairs_max"] = ms, int(out[3].max().item())
        row["kernel_statuses"] = out[1].cpu().tolist()
        if dense is not None:
            D3, D2 = up(dense[0]), up(dense[1])
            row["torch_pair_ms"] = timed(lambda: torch_eval(X0, D3, D2, 5.0), max(3, args.iters // 4))
            ms, (xt, steps) = wall(lambda: torch_lm(X0, D3, D2), max(2, args.set_iters // 2))
            row["torch_set_ms"], row["torch_set_steps"] = ms, int(steps)
            row["torch_vs_kernel_max_param_diff"] = float((xt - out[0]).abs().max().item())
            row["speedup_pair_vs_torch"] = row["torch_pair_ms"] / row["kernel_pair_ms"] if row["kernel_pair_ms"] > 0 else None
            row["speedup_set_vs_torch"] = row["torch_set_ms"] / row["kernel_set_ms"]
            cams = list(range(min(args.scipy_cameras, len(cors))))
        else:
            row["torch_pair_ms"] = row["torch_set_ms"] = None  # the batched baseline needs equal counts: not measured at this size
            cams = [c for c in range(len(cors)) if len(cors[c][0]) >= 20]
        ms, nfev = scipy_set(init, cors, cams)
        row["scipy_cameras_timed"], row["scipy_nfev"] = len(cams), nfev
        row["scipy_set_ms"] = ms * (len(cors) / len(cams) if dense is not None else 1.0)
        row["scipy_scaled_to_all_cameras"] = dense is not None and len(cams) < len(cors)
        row["speedup_set_vs_scipy"] = row["scipy_set_ms"] / row["kernel_set_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
