"""Cost of the colour (HardPhong) path against the soft silhouette on the same images: cfg2b shape (STICK, 4096 frames x 1 view @256^2)
and cfg3 shape (mouse, 256 frames x 18 views @256^2), the synthetic poses and camera ring of bench.py.  After warm-up the two calls
alternate on the same vertices (``engine.render_colour`` - setup, normals, background, tile kernel - and ``smil_silhouette_forward``
through ``engine.silhouette_forward``, projection excluded from both) and one JSON line per workload is printed: ms per call each,
the ratio, images/s and the colour output's bytes over its time.

    python3 tools/colour_probe.py
    rocprofv3 --kernel-trace --stats -d colour_prof -o colour -- python3 tools/colour_probe.py --reps 5
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from smilify_amd import engine, model_io, synthetic  # noqa: E402

WORKLOADS = {
    "cfg2b": dict(model="SMILy_STICK", frames=4096, views=1, S=256, radius=2.7),
    "cfg3": dict(model="SMILy_Mouse_static_joints", frames=256, views=18, S=256, radius=4.0),
}

ap = argparse.ArgumentParser()
ap.add_argument("--workload", action="append", choices=sorted(WORKLOADS))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
dev = torch.device("cuda:0")
for name in args.workload or sorted(WORKLOADS):
    w = WORKLOADS[name]
    t = model_io.load_model(os.path.join(REPO, "data", "models", w["model"] + ".npz"))
    dm = engine.DeviceModel(t, dev)
    frames, views, S = w["frames"], w["views"], w["S"]
    gen = torch.Generator().manual_seed(1234)
    pose, trans = synthetic.random_pose(frames, t.J, gen)
    out = engine.lbs_forward(dm, torch.zeros(t.nB, device=dev), pose.to(dev).contiguous(), trans=trans.to(dev).contiguous(), shared_beta=True,
                             trans_after_joints=True)
    verts = out["verts"].contiguous()
    R, T = synthetic.camera_ring(views, w["radius"], device=dev)
    cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 60.0, device=dev), None, views, S)
    ndc, _ = engine.project(cams, verts, want_yx=False)
    N = frames * views
    rgb = [0.0, 172.0 / 255.0, 223.0 / 255.0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_col = t_sil = 0.0
    for it in range(args.warmup + args.reps):
        ev[0].record()
        img = engine.render_colour(dm, cams, verts, rgb, verts_ndc=ndc)
        ev[1].record()
        sil = engine.silhouette_forward(dm, ndc, S)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            t_col += ev[0].elapsed_time(ev[1])
            t_sil += ev[1].elapsed_time(ev[2])
        del img, sil
    t_col /= args.reps
    t_sil /= args.reps
    out_bytes = N * 3 * S * S * 4
    print(json.dumps({"workload": name, "model": w["model"], "images": N, "S": S, "colour_ms": round(t_col, 4), "silhouette_fwd_ms": round(t_sil, 4),
                      "colour_over_silhouette": round(t_col / t_sil, 4), "colour_images_per_s": round(N / (t_col * 1e-3), 1),
                      "colour_output_GB_per_s": round(out_bytes / (t_col * 1e-3) / 1e9, 1), "reps": args.reps}), flush=True)
    del dm, verts, ndc
    torch.cuda.empty_cache()
