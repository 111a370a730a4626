"""Time per call of the rotation conversions (smilify_amd.rotations, csrc/rotations.hip) next to the same functions as compositions of
torch ops on the same device (tests/rotations_ref.py in float32, what a caller without pytorch3d writes today), forward and forward
plus backward, at n = 4096 x 55 rotations (a batch of 4096 poses of a 55-joint model) and sixteen times that.

Needs a GPU; writes profiles/rotations_probe.json (``--out``).  The parent of these kernels has none to compare with: the torch
composition is the baseline.

Method: that of tools/probelib.py, the kernel's and the composition's windows alternating.  Here: float32 storage; a window holds 20
to 2000 calls, sized from a first window of 10.  On the small size the figures are bounded by the host, not the device; the bytes
a call must move (inputs read once, outputs written once) are recorded with the rate they imply.

    python3 tools/rotations_probe.py
"""
import argparse
import json
import os
import sys

import probelib
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import rotations_cases as cases  # noqa: E402
import rotations_ref as ref  # noqa: E402
from smilify_amd import _lib, rotations  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rotations_probe.json"))
ap.add_argument("--window-ms", type=float, default=100.0, help="a timed window holds as many calls as fill this (20 to 2000 calls)")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="*", default=[4096 * 55, 4096 * 55 * 16])
args = ap.parse_args()
dev = torch.device("cuda:0")

# name -> (kernel path, torch composition, inputs of a case set, values per rotation read + written forward)
FUNCTIONS = {
    "rotation_6d_to_matrix": (rotations.rotation_6d_to_matrix, ref.rotation_6d_to_matrix, ("d6",), 6 + 9),
    "axis_angle_to_matrix": (rotations.axis_angle_to_matrix, ref.axis_angle_to_matrix, ("aa",), 3 + 9),
    "matrix_to_axis_angle": (rotations.matrix_to_axis_angle, ref.matrix_to_axis_angle, ("R",), 9 + 3),
    "rotation_6d_to_axis_angle": (rotations.rotation_6d_to_axis_angle, ref.rotation_6d_to_axis_angle, ("d6",), 6 + 3),
    "rotation_6d_distance": (rotations.rotation_6d_distance, ref.rotation_6d_distance, ("d6", "d6b"), 12 + 1),
}


def forward_of(fn, xs):
    return lambda: fn(*xs)


def forward_backward_of(fn, xs):
    leaves = [x.clone().requires_grad_(True) for x in xs]
    w = torch.ones_like(fn(*xs))

    def call():
        return torch.autograd.grad(fn(*leaves), leaves, w)
    return call


rows = []
for n in args.sizes:
    c = cases.regular(n)
    data = dict(d6=c["d6"], aa=c["aa"], R=c["R"], d6b=cases.regular(n, cases.REGULAR_SEED + 1)["d6"])
    data = {k: v.float().to(dev) for k, v in data.items()}
    for name, (kernel_fn, torch_fn, keys, values) in FUNCTIONS.items():
        xs = [data[k] for k in keys]
        for mode, make in (("forward", forward_of), ("forward_backward", forward_backward_of)):
            pair = {"kernel": make(kernel_fn, xs), "torch": make(torch_fn, xs)}
            probelib.warm_up(pair.values(), args.warmup)
            times, calls = probelib.alternate(pair, window_ms=args.window_ms, windows=args.windows, first=10, lo=20, hi=2000)
            moved = 4 * n * values * (2 if mode == "forward_backward" else 1)  # the backward reads and writes the mirror image
            row = dict(function=name, mode=mode, n=n, bytes_moved=moved, kernel_calls=calls["kernel"], torch_calls=calls["torch"])
            for who, t in times.items():
                row.update({f"{who}_{k}": v for k, v in t.items()})
            row["kernel_gb_per_s"] = moved / (row["kernel_ms"] * 1e-3) / 1e9
            row["torch_over_kernel"] = row["torch_ms"] / row["kernel_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)

probelib.write_result(args.out, dict(device=torch.cuda.get_device_name(0), library=_lib.load().smil_version().decode(), dtype="float32",
                                     window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, rows=rows))
