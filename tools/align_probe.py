"""Time per call of the 3-D alignment (smilify_amd.align, csrc/align.hip) next to the same computation composed from torch operations on
the same device (tests/align_ref.py: weighted Kabsch / Umeyama through torch.linalg.svd, float64, one problem at a time with the
status rule decided on the host - the shape of the reference's own per-sample MPJPE loop), at B = 64 and B = 1 problems of J = 55
joints.

Needs a GPU; writes profiles/align_probe.json (``--out``).  The parent of these kernels has none to compare with: the torch
composition is the baseline, and the ratios are recorded as they come out.

Every function is one STEP under its own time limit (``--step-seconds``), and the kernel's and the composition's windows alternate:
the runner and the method are those of tools/probelib.py.  Here: float32 storage; both paths are warmed up at both sizes first; a
window holds 3 to 20000 calls, sized from a first window of 3.  The figures include mask conversion and autograd bookkeeping: at
these sizes they measure launches and the host, not the device.

    python3 tools/align_probe.py
"""
import argparse
import os
import sys

import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["similarity_transform", "rigid_transform_robust", "pa_mpjpe"]
MODES = {"similarity_transform": "forward_backward", "rigid_transform_robust": "forward_backward", "pa_mpjpe": "forward"}
J = 55

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "align_probe.json"))
ap.add_argument("--window-ms", type=float, default=300.0, help="a timed window holds as many calls as fill this (3 to 20000 calls)")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="*", default=[64, 1])
ap.add_argument("--step-seconds", type=float, default=180.0, help="time limit of one step (a child process)")
ap.add_argument("--step", choices=STEPS, help="(internal) run this step in this process and print its rows")
args = ap.parse_args()


def run_step(name):
    import torch

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import align_cases as cases
    import align_ref as ref
    from smilify_amd import align

    dev = torch.device("cuda:0")

    def pair_for(B):
        c = cases.regular(B, J, seed=B, weights=None)
        src, dst, mask = c["src"].float().to(dev), c["dst"].float().to(dev), c["mask"].to(dev)
        src64, dst64 = src.double(), dst.double()

        def forward_backward(fn, a, b):
            leaves = [a.clone().requires_grad_(True), b.clone().requires_grad_(True)]

            def call():
                x = fn(*leaves)
                return torch.autograd.grad(x.R.sum() + x.t.sum() + x.s.sum(), leaves)
            return call

        robust = dict(robust_iters=10, robust_scale=0.05)
        if name == "similarity_transform":
            return (forward_backward(lambda s, d: align.similarity_transform(s, d, mask=mask), src, dst),
                    forward_backward(lambda s, d: ref.similarity_transform(s, d, mask=mask)[0], src64, dst64))
        if name == "rigid_transform_robust":
            return (forward_backward(lambda s, d: align.rigid_transform(s, d, mask=mask, **robust), src, dst),
                    forward_backward(lambda s, d: ref.rigid_transform(s, d, mask=mask, **robust)[0], src64, dst64))
        return lambda: align.pa_mpjpe(src, dst, mask), lambda: ref.pa_mpjpe(src64, dst64, mask)

    pairs = {B: dict(zip(("kernel", "torch"), pair_for(B))) for B in args.batches}
    probelib.warm_up([fn for pair in pairs.values() for fn in pair.values()], args.warmup)  # every shape of the timed windows, before any of them
    for B, pair in pairs.items():
        times, calls = probelib.alternate(pair, window_ms=args.window_ms, windows=args.windows, first=3, lo=3, hi=20000)
        row = dict(function=name, mode=MODES[name], B=B, J=J, kernel_calls=calls["kernel"], torch_calls=calls["torch"])
        for who, t in times.items():
            row.update({f"{who}_{k}": v for k, v in t.items()})
        row["torch_over_kernel"] = row["torch_ms"] / row["kernel_ms"]
        probelib.emit_row(row)
    probelib.emit_device(torch.cuda.get_device_name(0))


if args.step:
    run_step(args.step)
    sys.exit(0)

forward = ["--window-ms", str(args.window_ms), "--windows", str(args.windows), "--warmup", str(args.warmup), "--batches"] + [str(b) for b in args.batches]
rows, failed, device, finished = probelib.run_steps(os.path.abspath(__file__), STEPS, forward, args.step_seconds)
probelib.write_result(args.out, dict(device=device, dtype="float32",
                                     baseline="tests/align_ref.py on the device (float64, torch.linalg.svd, one problem at a time)",
                                     window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, failed=failed,
                                     not_measured=STEPS[finished:], rows=rows))
sys.exit(1 if failed else 0)
