"""Times of the mesh-free joints path (smilify_amd/csrc/joints.hip) next to what the library offered for the same task before it.

(a) ``SMAL.joints`` forward + backward against ``SMAL.__call__`` forward + backward with only the joints' gradient upstream, at
    B = 4096 frames, on STICK (55 joints, regressed) and the mouse (31 static joints).
(b) One ``KeypointFitter3D.fit_step`` at N = 4096 and N = 131072 frames against the same iteration built from ``SMAL.__call__`` +
    ``keypoint_losses.keypoint_loss_3d`` + autograd + ``torch.optim.Adam`` (per-frame pose and translation, shared shape), its
    frames cut into chunks of ``--chunk`` because it holds every vertex of a chunk; gradients of the shared shape add up over the
    chunks, one optimiser step per iteration.  The two do not minimise the same number (window means against a pooled mean): the
    baseline stands for the work such an iteration costs, not for its value.

Needs a GPU; writes profiles/joints_probe.json (``--out``).  Method: that of tools/probelib.py, the two paths' windows alternating.
Here: a window holds 2 to 500 calls, sized from a first window of 2.

    python3 tools/joints_probe.py
"""
import argparse
import json
import os
import sys

import probelib
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import _lib, keypoint_losses, model_io  # noqa: E402
from smilify_amd.fit_keypoints3d import KeypointFitter3D  # noqa: E402
from smilify_amd.smal_torch import SMAL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "joints_probe.json"))
ap.add_argument("--window-ms", type=float, default=300.0)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--fit-sizes", type=int, nargs="*", default=[4096, 131072])
ap.add_argument("--chunk", type=int, default=4096, help="frames per chunk of the baseline iteration")
args = ap.parse_args()
dev = torch.device("cuda:0")
MODELS = {"stick": "SMILy_STICK.npz", "mouse": "SMILy_Mouse_static_joints.npz"}


def compare(row, pair):
    probelib.warm_up(pair.values(), args.warmup)
    times, calls = probelib.alternate(pair, window_ms=args.window_ms, windows=args.windows, first=2, lo=2, hi=500)
    for who, t in times.items():
        row.update({f"{who}_{k}": v for k, v in t.items()}, **{f"{who}_calls": calls[who]})
    row["baseline_over_joints"] = row["baseline_ms"] / row["joints_ms"]
    row["peak_memory_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20
    print(json.dumps(row), flush=True)
    return row


rows = []
for name, file in MODELS.items():
    t = model_io.load_model(os.path.join(REPO, "data", "models", file))
    smal = SMAL(dev, tables=t)
    g = torch.Generator().manual_seed(1)
    B, J = args.batch, t.J
    leaf = lambda x: x.to(dev).requires_grad_()  # noqa: E731
    beta, theta, trans = leaf(0.3 * torch.randn(1, t.nB, generator=g)), leaf(0.3 * torch.randn(B, J, 3, generator=g)), leaf(0.1 * torch.randn(B, 3, generator=g))
    dj = torch.randn(B, J, 3, generator=g).to(dev)

    def fb_joints():
        return torch.autograd.grad(smal.joints(beta, theta, trans), (beta, theta, trans), dj)

    def fb_call():
        return torch.autograd.grad(smal(beta, theta, trans)[1], (beta, theta, trans), dj)

    torch.cuda.reset_peak_memory_stats()
    rows.append(compare(dict(what="joints_forward_backward", model=name, B=B, J=J, V=t.V, bytes_out_joints=B * J * 12, bytes_out_verts=B * t.V * 12),
                        {"joints": fb_joints, "baseline": fb_call}))

    for N in args.fit_sizes:
        target = (0.5 * torch.randn(N, J, 3, generator=g)).to(dev)
        fitter = KeypointFitter3D(dev, target, tables=t)
        fitter.begin_stage(5e-3)
        del smal
        smal = SMAL(dev, tables=t)
        p_beta = torch.zeros(1, t.nB, device=dev, requires_grad=True)
        p_theta, p_trans = fitter._pose.clone().requires_grad_(), torch.zeros(N, 3, device=dev, requires_grad=True)
        opt = torch.optim.Adam([p_beta, p_theta, p_trans], lr=5e-3, betas=(0.5, 0.999))
        chunk = min(args.chunk, N)

        def step_fitter():
            return fitter.fit_step(40.0, w_betas=1.5, w_limit=100.0, w_splay=0.1, w_temp=30.0)

        def step_baseline():
            opt.zero_grad(set_to_none=False)
            for s in range(0, N, chunk):
                joints = smal(p_beta, p_theta[s:s + chunk], p_trans[s:s + chunk])[1]
                (40.0 * keypoint_losses.keypoint_loss_3d(joints, target[s:s + chunk], None, reduction="pooled")).backward()
            opt.step()

        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        rows.append(compare(dict(what="fit_step", model=name, N=N, J=J, V=t.V, baseline_chunk=chunk), {"joints": step_fitter, "baseline": step_baseline}))
        del fitter, opt, p_theta, p_trans, target
        torch.cuda.empty_cache()

probelib.write_result(args.out, dict(device=torch.cuda.get_device_name(0), library=_lib.load().smil_version().decode(), window_ms=args.window_ms,
                                     windows=args.windows, warmup=args.warmup, rows=rows))
