"""Times of the mesh-free joints path (smilify_amd/csrc/joints.hip) next to what the library offered for the same task before it.

(a) ``SMAL.joints`` forward + backward against ``SMAL.__call__`` forward + backward with only the joints' gradient upstream, at
    B = 4096 frames, on STICK (55 joints, regressed) and the mouse (31 static joints).
(b) One ``KeypointFitter3D.fit_step`` at N = 4096 and N = 131072 frames against the same iteration built from ``SMAL.__call__`` +
    ``keypoint_losses.keypoint_loss_3d`` + autograd + ``torch.optim.Adam`` (per-frame pose and translation, shared shape), its
    frames cut into chunks of ``--chunk`` because it holds every vertex of a chunk; gradients of the shared shape add up over the
    chunks, one optimiser step per iteration.  The two do not minimise the same number (window means against a pooled mean): the
    baseline stands for the work such an iteration costs, not for its value.

Needs a GPU; writes profiles/joints_probe.json (``--out``).  Method: every path is warmed up at every size; a window is as many
back-to-back calls as fill ``--window-ms`` (2 to 500, sized from a first window of 2) between two device events, ended by a
synchronise; the two paths' windows ALTERNATE, ``--windows`` of each; median, min and max of the per-call time are recorded.  The times
are those of the whole Python call (allocation, autograd bookkeeping and launches included).

    python3 tools/joints_probe.py
"""
import argparse
import json
import os
import statistics
import sys

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


def window(fn, calls):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / calls


def compare(row, pair):
    for fn in pair.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    calls = {who: int(min(500, max(2, args.window_ms / max(window(fn, 2), 1e-6)))) for who, fn in pair.items()}
    times = {who: [] for who in pair}
    for _ in range(args.windows):
        for who, fn in pair.items():
            times[who].append(window(fn, calls[who]))
    for who, t in times.items():
        row[f"{who}_ms"], row[f"{who}_ms_min"], row[f"{who}_ms_max"], row[f"{who}_calls"] = statistics.median(t), min(t), max(t), calls[who]
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

result = dict(device=torch.cuda.get_device_name(0), library=_lib.load().smil_version().decode(), window_ms=args.window_ms, windows=args.windows,
              warmup=args.warmup, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(f"wrote {args.out}")
