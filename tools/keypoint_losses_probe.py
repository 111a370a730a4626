"""Time per call, forward plus backward, of the keypoint and triangulation losses (smilify_amd.keypoint_losses,
csrc/keypoint_losses.hip) next to the same computation composed from torch operations on the same device (tests/keypoint_losses_ref.py:
float64 arithmetic on the float32 inputs, what the kernels evaluate; like the reference it asks the device whether anything is valid,
which synchronises), at B = 64 and B = 1 samples of V = 6 views, J = 55 joints, S = 256.

Needs a GPU; writes profiles/keypoint_losses_probe.json (``--out``).  The parent of these kernels has none to compare with: the
torch composition is the baseline, and the ratios are recorded as they come out, below 1 included.

Every function is one STEP under its own time limit (``--step-seconds``), and the kernel's and the composition's windows alternate:
the runner and the method are those of tools/probelib.py.  Here: float32 storage; both paths are warmed up at both sizes first; a
window (half a second by default) holds 20 to 20000 calls, sized from a first window of 10.  The figures include mask conversion
and autograd bookkeeping: at these sizes (a few hundred KB) they measure launches and the host, not the device.

    python3 tools/keypoint_losses_probe.py
"""
import argparse
import os
import sys

import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["keypoint_loss_2d", "keypoint_loss_3d", "project_joints_to_views", "multiview_keypoint_loss", "triangulate_joints_dlt",
         "triangulation_consistency_loss"]
V, J = 6, 55

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keypoint_losses_probe.json"))
ap.add_argument("--window-ms", type=float, default=500.0, help="a timed window holds as many calls as fill this (20 to 20000 calls)")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[64, 1])
ap.add_argument("--step-seconds", type=float, default=240.0, help="time limit of one step (a child process)")
ap.add_argument("--step", choices=STEPS, help="(internal) run this step in this process and print its rows")
args = ap.parse_args()


def run_step(name):
    import torch

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import keypoint_losses_cases as cases
    import keypoint_losses_ref as ref
    from smilify_amd import keypoint_losses as kl

    dev = torch.device("cuda:0")

    def pair_for(B):
        """(kernel call, torch call, names of the leaves): each runs forward and backward"""
        c = cases.regular(B, V, J, seed=B)
        g = {k: (v.float() if v.is_floating_point() else v).to(dev) for k, v in c.items() if isinstance(v, torch.Tensor)}
        S = c["S"]
        gen = torch.Generator().manual_seed(6000)
        kp = (c["observed"] + 0.005 * torch.randn(c["observed"].shape, generator=gen, dtype=torch.float64)).float().to(dev)
        pred3, target3, vis3 = (t.to(dev) for t in cases.points_3d(B, J))
        pred3, target3 = pred3.float(), target3.float()
        cams = ("R", "T", "fov")
        table = {
            "keypoint_loss_2d": (("proj",), lambda p: kl.keypoint_loss_2d(p, g["target"], g["visibility"]),
                                 lambda p: ref.keypoint_loss_2d(p, g["target"], g["visibility"])),
            "keypoint_loss_3d": (("pred3",), lambda p: kl.keypoint_loss_3d(p, target3, vis3), lambda p: ref.keypoint_loss_3d(p, target3, vis3)),
            "project_joints_to_views": (("joints",) + cams, lambda j, R, T, f: kl.project_joints_to_views(j, R, T, f, S, g["aspect"]),
                                        lambda j, R, T, f: ref.project_joints_to_views(j, R, T, f, S, g["aspect"])),
            "multiview_keypoint_loss": (("joints",) + cams,
                                        lambda j, R, T, f: kl.multiview_keypoint_loss(j, R, T, f, g["target"], g["visibility"], S, aspect_ratio=g["aspect"]),
                                        lambda j, R, T, f: ref.multiview_keypoint_loss(j, R, T, f, g["target"], g["visibility"], S, g["aspect"])),
            "triangulate_joints_dlt": (cams, lambda R, T, f: kl.triangulate_joints_dlt(kp, g["visibility"], R, T, f, S, aspect_ratio=g["aspect"])[0],
                                       lambda R, T, f: ref.triangulate_joints_dlt(kp, g["visibility"], R, T, f, S, g["aspect"])[0]),
            "triangulation_consistency_loss": (cams, lambda R, T, f: kl.triangulation_consistency_loss(kp, g["visibility"], g["joints"], R, T, f, S,
                                                                                                      aspect_ratio=g["aspect"]),
                                               lambda R, T, f: ref.triangulation_consistency_loss(kp, g["visibility"], g["joints"], R, T, f, S, g["aspect"])),
        }
        g["pred3"] = pred3
        keys, kernel_fn, torch_fn = table[name]

        def forward_backward(fn):
            leaves = [g[k].clone().requires_grad_(True) for k in keys]
            w = torch.ones_like(fn(*leaves)).detach()
            return lambda: torch.autograd.grad(fn(*leaves), leaves, w)
        return forward_backward(kernel_fn), forward_backward(torch_fn)

    pairs = {B: dict(zip(("kernel", "torch"), pair_for(B))) for B in args.batches}
    probelib.warm_up([fn for pair in pairs.values() for fn in pair.values()], args.warmup)  # every shape of the timed windows, before any of them
    for B, pair in pairs.items():
        times, calls = probelib.alternate(pair, window_ms=args.window_ms, windows=args.windows, first=10, lo=20, hi=20000)
        row = dict(function=name, mode="forward_backward", B=B, V=V, J=J, S=cases.S, kernel_calls=calls["kernel"], torch_calls=calls["torch"])
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
                                     baseline="tests/keypoint_losses_ref.py on the device (float64 arithmetic, torch.linalg.solve)",
                                     window_ms=args.window_ms, windows=args.windows, warmup=args.warmup, failed=failed,
                                     not_measured=STEPS[finished:], rows=rows))
sys.exit(1 if failed else 0)
