"""Cost of ``engine.render_fragments`` next to ``engine.render_colour`` on the same images at cfg2b's shape (STICK, 4096 frames x 1 view
@256^2, the synthetic poses and camera ring of bench.py).  After warm-up the three calls alternate on the same vertices - colour
(setup, normals, background, tile kernel), fragments with all four outputs, fragments with ``dist`` only; projection excluded from all -
and one JSON line is printed: ms per call each, the ratios to colour and the outputs' bytes over their time.

``--package-root DIR`` times the ``smilify_amd`` of another checkout (built there): the parent commit's ``render_colour`` is the
comparison value for the colour path, which this kernel's tile sweep was cut out of; a tree without ``render_fragments`` gives the
colour figure alone.

    python3 tools/fragments_probe.py
    python3 tools/fragments_probe.py --package-root ../parent_checkout
"""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
ROOT = os.path.abspath(args.package_root)
sys.path.insert(0, ROOT)
from smilify_amd import engine, model_io, synthetic  # noqa: E402

dev = torch.device("cuda:0")
t = model_io.load_model(os.path.join(ROOT, "data", "models", "SMILy_STICK.npz"))
dm = engine.DeviceModel(t, dev)
frames, views, S = args.frames, 1, 256
gen = torch.Generator().manual_seed(1234)
pose, trans = synthetic.random_pose(frames, t.J, gen)
out = engine.lbs_forward(dm, torch.zeros(t.nB, device=dev), pose.to(dev).contiguous(), trans=trans.to(dev).contiguous(), shared_beta=True,
                         trans_after_joints=True)
verts = out["verts"].contiguous()
R, T = synthetic.camera_ring(views, 2.7, device=dev)
cams = engine.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 60.0, device=dev), None, views, S)
ndc, _ = engine.project(cams, verts, want_yx=False)
N = frames * views
rgb = [0.0, 172.0 / 255.0, 223.0 / 255.0]
has_fragments = hasattr(engine, "render_fragments")
calls = [("colour", lambda: engine.render_colour(dm, cams, verts, rgb, verts_ndc=ndc))]
if has_fragments:
    calls += [("fragments_all", lambda: engine.render_fragments(dm, cams, verts, verts_ndc=ndc)),
              ("fragments_dist", lambda: engine.render_fragments(dm, cams, verts, verts_ndc=ndc, want=("dist",)))]
ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
ms = [0.0] * len(calls)
for it in range(args.warmup + args.reps):
    ev[0].record()
    for k, (_, call) in enumerate(calls):
        res = call()
        ev[k + 1].record()
        del res
    torch.cuda.synchronize()
    if it >= args.warmup:
        for k in range(len(calls)):
            ms[k] += ev[k].elapsed_time(ev[k + 1])
ms = [m / args.reps for m in ms]
pix_bytes = {"colour": 12, "fragments_all": 24, "fragments_dist": 4}
line = {"workload": "cfg2b", "model": "SMILy_STICK", "images": N, "S": S, "package_root": os.path.relpath(ROOT), "reps": args.reps,
        "version": engine._lib.load().smil_version().decode()}
for (name, _), m in zip(calls, ms):
    line[name + "_ms"] = round(m, 4)
    line[name + "_output_GB_per_s"] = round(N * S * S * pix_bytes[name] / (m * 1e-3) / 1e9, 1)
    if name != "colour":
        line[name + "_over_colour"] = round(m / ms[0], 4)
print(json.dumps(line), flush=True)
