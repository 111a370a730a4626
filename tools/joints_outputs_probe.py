"""Every output of the mesh-free joints entry points and of the multi-tensor Adam steps from seeded inputs, as .npy files: run once
per build of the library (``SMILFIT_LIB`` selects one, smilify_amd/_lib.py) and compare the two directories bit for bit.  For
changes to joints.hip / chain.h / fit.hip's Adam that must not change a single bit: the joint kernels use no atomics on their
outputs, so two builds that compute the same thing agree exactly.

    SMILFIT_LIB=/path/to/parent/libsmilfit.so python3 tools/joints_outputs_probe.py --out /tmp/j_a
    python3 tools/joints_outputs_probe.py --out /tmp/j_b
    python3 tools/joints_outputs_probe.py --compare /tmp/j_a /tmp/j_b

Covers smil_joints_forward, smil_joints_backward, smil_kp3d_fit_eval, smil_kp2d_fit_eval, smil_adam_step_multi_bc64 and
smil_adam_step_multi.  Models: procedural tubes of 3, 65, 147 and 250 joints (65 also with static joints), STICK and the mouse
(static joints) - one to four joints per lane, and LDS above 64 KB at 250 joints; B = 2 and 7, and 4099 frames on the synthetic
model (the block loop and the last block's sum); per-frame and shared beta / logscale / btrans, each with and without ``theta_mask``;
robust scales zero and positive; 1 and 3 views with camera tables of 1, ``views`` and ``N * views`` rows; the 3-D term beside
the 2-D one; frame 0 with nothing visible.
"""
import argparse
import os
import sys

import numpy as np
import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="directory the .npy files are written to")
ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare two such directories instead of running anything")
ap.add_argument("--models", default="j3,mouse,stick,j65,j65_static,j147,j250")
ap.add_argument("--frames", default="2,7")
ap.add_argument("--long", type=int, default=4099, help="frames of the one long case on the synthetic model (0: none)")
args = ap.parse_args()

if args.compare:
    a, b = (probelib.load_arrays(d) for d in args.compare)
    only, changed = probelib.differing(a, b)
    bad = [("only in one directory", n + ".npy") for n in only]
    for n in changed:
        x, y = a[n], b[n]
        bad.append((n + ".npy", float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape else "shape"))
    print(f"{len(a)} / {len(b)} arrays, bit for bit: {len(bad)} differ")
    for x in bad:
        print("DIFFERS", x)
    sys.exit(1 if bad or not a else 0)

import torch  # noqa: E402

from smilify_amd import cameras as cam_mod  # noqa: E402
from smilify_amd import engine as eng  # noqa: E402
from smilify_amd import model_io  # noqa: E402
from smilify_amd.joints import JointTables  # noqa: E402

DEV = "cuda:0"
S = 64
os.makedirs(args.out, exist_ok=True)
n_saved = 0


def save(tag, d):
    global n_saved
    for k, v in d.items():
        if v is not None:
            assert v.dtype == torch.float32, (tag, k, v.dtype)
            np.save(os.path.join(args.out, f"{tag}.{k}.npy"), v.detach().cpu().numpy())
            n_saved += 1


def get_tables(key):
    if key.startswith("j"):
        return model_io.synthetic_model(V_side=6, J=int(key[1:].split("_")[0]), nB=3, seed=5, static_joints=key.endswith("_static"))
    if key == "synthetic":
        return model_io.synthetic_model()
    return model_io.load_model(os.path.join(REPO, "data", "models", {"stick": "SMILy_STICK", "mouse": "SMILy_Mouse_static_joints"}[key] + ".npz"))


def cameras(B, views, rows, g, principal):
    """``views`` views whose tables hold ``rows`` rows (1, views or B * views)."""
    R, T = cam_mod.look_at_view_transform(3.0, 10.0, np.linspace(0, 300, views), device="cpu")
    rep = rows // views if rows >= views else 1
    R, T = R.repeat(rep, 1, 1)[:rows], T.repeat(rep, 1)[:rows] + 0.05 * torch.randn(rows, 3, generator=g)
    fov = 50.0 + 10.0 * torch.rand(rows, generator=g)
    pp = (0.05 * torch.randn(rows, 2, generator=g)).contiguous().to(DEV) if principal else None
    return eng.CameraSet(R.contiguous().to(DEV), T.contiguous().to(DEV), fov.to(DEV), None, views, S, pp)


def run_case(key, B, full=True):
    t = get_tables(key)
    jt = eng.DeviceJointTables(JointTables.from_tables(t), DEV)
    J, nB = jt.J, jt.nB
    g = torch.Generator().manual_seed(4000 + 13 * B + J)
    rnd = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g)).to(DEV)  # noqa: E731
    theta, trans = rnd(B, J, 3, s=0.25), rnd(B, 3, s=0.1)
    mask = (torch.rand(J, 3, generator=g) > 0.3).float().to(DEV)
    d_joints = rnd(B, J, 3)
    Jc = min(J, 12)
    canon = torch.randperm(J, generator=g)[:Jc].to(torch.int32).to(DEV)
    wj = (0.5 + torch.rand(Jc, generator=g, dtype=torch.float64)).to(DEV)
    target3d = rnd(B, Jc, 3, s=0.3)
    target3d[B - 1, 0, 1] = float("nan")
    vis3d = (torch.rand(B, Jc, generator=g) > 0.2).to(torch.uint8).to(DEV)
    vis3d[0] = 0  # frame 0: nothing visible
    for shared in ((False, True) if full else (True,)):
        beta = rnd(nB, s=0.4) if shared else rnd(B, nB, s=0.4)
        ls, bt = (rnd(J, 3, s=0.05), rnd(J, 3, s=0.02)) if shared else (rnd(B, J, 3, s=0.05), rnd(B, J, 3, s=0.02))
        kw = dict(trans=trans, logscale=ls, btrans=bt, theta_mask=mask if shared == (B % 2 == 1) else None)  # (both axes: mask with shared tables at odd B, with per-frame ones at even B)
        tag = f"{key}.B{B}.{'shared' if shared else 'frame'}"
        for after in ((True, False) if full else (True,)):
            joints, new_J = eng.joints_forward(jt, beta, theta, trans_after_joints=after, **kw)
            save(f"{tag}.fwd{int(after)}", dict(joints=joints, new_J=new_J))
            save(f"{tag}.bwd{int(after)}", eng.joints_backward(jt, d_joints, beta, theta, trans_after_joints=after, **kw))
        cfg = eng.fit_config(B, J, nB, 3, [0.0] * 6)  # windows of three frames: the last one is short

        def outputs(views=0):
            o = dict(objs=torch.zeros(16, device=DEV), d_pose=torch.empty(B, J, 3, device=DEV), d_trans=torch.empty(B, 3, device=DEV),
                     d_betas=torch.empty_like(beta) if nB else None, d_logscale=torch.empty_like(ls), d_btrans=torch.empty_like(bt),
                     joints_out=torch.empty(B, J, 3, device=DEV))
            if views:
                o["yx_out"] = torch.empty(B, views, Jc, 2, device=DEV)
            return o

        for sigma in (0.0, 0.05):
            o = outputs()
            eng.kp3d_fit_eval(cfg, jt, 1.5, sigma, canon, target3d, vis3d, wj, beta, theta, trans, ls, bt, kw["theta_mask"], **o)
            save(f"{tag}.kp3d.s{sigma}", o)
        for views, rows, sigma_px, beside in ((1, 1, 0.0, False), (3, 3, 4.0, True), (3, 3 * B, 0.0, False)) if full else ((3, 3, 4.0, True),):
            cams = cameras(B, views, rows, g, principal=rows == 3)
            target2d = (S * torch.rand(B, views, Jc, 2, generator=g)).to(DEV)
            target2d[B - 1, 0, 0, 0] = float("nan")
            vis2d = (torch.rand(B, views, Jc, generator=g) > 0.2).to(torch.uint8).to(DEV)
            vis2d[0] = 0
            conf = torch.rand(B, views, Jc, generator=g).to(DEV)
            conf[B - 1, 0, 1] = 0.0
            o = outputs(views)
            eng.kp2d_fit_eval(cfg, jt, cams, 2.0, sigma_px, canon, target2d, vis2d, conf, wj, beta, theta, trans, ls, bt, kw["theta_mask"],
                              w_k3d=1.5 if beside else 0.0, robust_scale=0.05, target3d=target3d if beside else None,
                              visibility3d=vis3d if beside else None, **o)
            save(f"{tag}.kp2d.v{views}.r{rows}", o)
    torch.cuda.synchronize()


def run_adam():
    g = torch.Generator().manual_seed(11)
    for name, step_fn in (("adam_multi", eng.adam_step_multi), ("adam_multi_bc64", eng.adam_step_multi_bc64)):
        state = [[(s * torch.randn(n, generator=g)).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
                 for n, s in ((5, 0.1), (1000, 1.0), (70001, 0.02))]
        for step in (1, 2, 3):
            grads = [(torch.randn(p.numel(), generator=g) * (1e3 if k == 1 else 1.0)).to(DEV) for k, (p, _, _) in enumerate(state)]
            step_fn([(p, gr, m, v, 5e-3 * (k + 1), step) for k, ((p, m, v), gr) in enumerate(zip(state, grads))], 0.5, 0.999, 1e-8)
        for k, (p, m, v) in enumerate(state):
            save(f"{name}.t{k}", dict(param=p, exp_avg=m, exp_avg_sq=v))
    torch.cuda.synchronize()


for key in args.models.split(","):
    for B in (int(x) for x in args.frames.split(",")):
        run_case(key, B)
        print(f"{key} B={B}: {n_saved} arrays so far", flush=True)
if args.long:
    run_case("synthetic", args.long, full=False)
    print(f"synthetic B={args.long}: {n_saved} arrays so far", flush=True)
run_adam()
print(f"{n_saved} arrays in {args.out} (library: {os.environ.get('SMILFIT_LIB', 'the default build')})")
