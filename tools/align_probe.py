"""Time per call of the 3-D alignment (smilify_amd.align, csrc/align.hip) next to the same computation composed from torch operations on
the same device (tests/align_ref.py: weighted Kabsch / Umeyama through torch.linalg.svd, float64, one problem at a time with the
status rule decided on the host - the shape of the reference's own per-sample MPJPE loop), at B = 64 and B = 1 problems of J = 55
joints.

Needs a GPU; writes profiles/align_probe.json (``--out``).  The parent of these kernels has none to compare with: the torch
composition is the baseline, and the ratios are recorded as they come out.

Every function is one STEP: a child process of its own under its own time limit (``--step-seconds``), so a step that hangs or
faults ends alone; the parent never opens the device, and after a step that failed it starts no other.

Method (per step): float32 storage.  Both paths are warmed up at both sizes first.  A window is as many back-to-back calls as fill
``--window-ms`` (3 to 20000 calls, sized from a first window of 3) between two device events, ended by a synchronise; the kernel's and
the composition's windows ALTERNATE, ``--windows`` of each, and the median and the spread (min, max) of the per-call time are
recorded.  The figures are times of the whole Python call - argument checks, mask conversion, output allocation, autograd
bookkeeping and launch latency included: at these sizes they measure launches and the host, not the device.

    python3 tools/align_probe.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

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

    def window(fn, calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / calls

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
    for pair in pairs.values():  # every shape of the timed windows, before any of them
        for fn in pair.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    for B, pair in pairs.items():
        calls = {who: int(min(20000, max(3, args.window_ms / max(window(fn, 3), 1e-6)))) for who, fn in pair.items()}
        times = {"kernel": [], "torch": []}
        for _ in range(args.windows):
            for who, fn in pair.items():
                times[who].append(window(fn, calls[who]))
        row = dict(function=name, mode=MODES[name], B=B, J=J, kernel_calls=calls["kernel"], torch_calls=calls["torch"])
        for who, t in times.items():
            row[f"{who}_ms"] = statistics.median(t)
            row[f"{who}_ms_min"], row[f"{who}_ms_max"] = min(t), max(t)
        row["torch_over_kernel"] = row["torch_ms"] / row["kernel_ms"]
        print("ROW " + json.dumps(row), flush=True)
    print("DEVICE " + json.dumps(torch.cuda.get_device_name(0)), flush=True)


if args.step:
    run_step(args.step)
    sys.exit(0)

rows, failed, device = [], [], None
for step in STEPS:
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--window-ms", str(args.window_ms), "--windows", str(args.windows),
           "--warmup", str(args.warmup), "--batches"] + [str(b) for b in args.batches]
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
        status = done.returncode
        out = done.stdout
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

result = dict(device=device, dtype="float32", baseline="tests/align_ref.py on the device (float64, torch.linalg.svd, one problem at a time)",
              window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, failed=failed,
              not_measured=STEPS[len(rows) // max(1, len(args.batches)):], rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(f"wrote {args.out}")
sys.exit(1 if failed else 0)
