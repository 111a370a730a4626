"""Every output of the rasteriser entry points from seeded scenes, as .npy files: run once per build of the library
(``SMILFIT_LIB`` selects one, smilify_amd/_lib.py) and compare the directories bit for bit.  For changes to raster.hip, its
headers or shade.hip that must not change a single bit (kernels whose source moved without their arithmetic moving).

    SMILFIT_LIB=smilify_amd/lib/libsmilfit_parent.so python3 tools/raster_outputs_probe.py --out /tmp/ras_a
    SMILFIT_LIB=smilify_amd/lib/libsmilfit_parent.so python3 tools/raster_outputs_probe.py --out /tmp/ras_a2
    python3 tools/raster_outputs_probe.py --out /tmp/ras_b
    python3 tools/raster_outputs_probe.py --compare /tmp/ras_a /tmp/ras_b --baseline /tmp/ras_a2

Per case ``silhouette_forward``, ``silhouette_backward``, ``silhouette_l1_fused`` (silhouette, per-image loss, ``d_ndc``),
``raster_stats`` and ``render_colour`` (image, pix_to_face).  Cases: STICK and the mouse; S = 64 and 256; N = 3 and N = 64 images
(from 64 on the fused entry point flushes its gradient as packed fixed point); K = 100 and K = 4 (tiles truncate, select and cut
tie groups); both tie rules; and one scene per model whose mesh crosses z_clip.

``--compare A B`` wants every array bit-equal.  The one exception is ``d_ndc`` of a launch below 64 images, whose flush ends in
float atomics from several workgroups: with ``--baseline A2 [A3 ...]`` (further runs of A's library) such an array passes if the
runs of A's library differ among themselves as well and B is no farther from A than the farthest two of them are from each other,
relative to the array's largest entry; if all runs of A's library agree bit for bit it must agree between A and B too.  The arrays
that took this path are named.  Every other array that differs is reported, with the same two figures beside it.
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
ap.add_argument("--baseline", metavar="DIR", nargs="+", help="with --compare A B: further runs of A's library (the run-to-run difference)")
ap.add_argument("--models", default="stick,mouse")
ap.add_argument("--sizes", default="64,256")
ap.add_argument("--images", default="3,64")
ap.add_argument("--faces-per-pixel", default="100,4")
args = ap.parse_args()


def rel_diff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / (np.abs(a.astype(np.float64)).max() + 1e-300))


if args.compare:
    a, b = (probelib.load_arrays(d) for d in args.compare)
    baseline = [probelib.load_arrays(d) for d in args.baseline or []]
    only, changed = probelib.differing(a, b)
    bad, took, worst = [(n + ".npy", "only in one directory") for n in only], [], (0.0, 0.0, "")
    for n in changed:
        x, y = a[n], b[n]
        if x.shape != y.shape or not baseline:
            bad.append((n + ".npy", "shape" if x.shape != y.shape else rel_diff(x, y)))
            continue
        runs = [x] + [r[n] for r in baseline]
        own = max(rel_diff(p, q) for i, p in enumerate(runs) for q in runs[i + 1:])
        new = rel_diff(x, y)
        small_launch_d_ndc = n.endswith("d_ndc") and ".N64." not in n  # (the clip scenes are three images)
        runs_agree = not any(probelib.differing({n: x}, {n: r})[1] for r in runs[1:])
        if not small_launch_d_ndc or runs_agree or not new <= own:
            bad.append((n + ".npy", f"differs by {new:.3e} of its largest entry; the runs of the first library among themselves by {own:.3e}"))
        else:
            took.append(f"{n}.npy: {new:.3e} (run-to-run {own:.3e})")
            if new > worst[0]:
                worst = (new, own, n + ".npy")
    print(f"{len(set(a) | set(b))} arrays: {len(set(a) & set(b)) - len(changed)} bit-equal, {len(took)} d_ndc of launches below 64 images within the "
          f"first library's own run-to-run difference, {len(bad)} differ")
    for x in took:
        print("RUN-TO-RUN", x)
    if took:
        print(f"largest accepted difference {worst[0]:.3e} (run-to-run {worst[1]:.3e}) in {worst[2]}")
    for x in bad:
        print("DIFFERS", x)
    sys.exit(1 if bad or not a else 0)

import torch  # noqa: E402

from smilify_amd import engine as eng  # noqa: E402
from smilify_amd import model_io, synthetic  # noqa: E402

DEV = "cuda:0"
os.makedirs(args.out, exist_ok=True)
n_saved = 0


def save(tag, **arrays):
    global n_saved
    for k, v in arrays.items():
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        np.save(os.path.join(args.out, f"{tag}.{k}.npy"), a)
        n_saved += 1


def scene(t, dm, N, S, seed):
    """N images of one camera ring: projected vertices of a random pose, binary targets from a second one."""
    views = 3 if N % 3 == 0 else 4
    frames = N // views
    assert frames * views == N
    R, T = synthetic.camera_ring(views, 2.7, device=DEV)
    cams = eng.CameraSet(R.contiguous(), T.contiguous(), torch.full((1,), 60.0, device=DEV), None, views, S)
    out = []
    for s in (seed, seed + 10 ** 6):
        g = torch.Generator().manual_seed(s)
        pose, trans = synthetic.random_pose(frames, t.J, g)
        betas = 0.5 * torch.randn(t.nB, generator=g)
        lbs = eng.lbs_forward(dm, betas.to(DEV), pose.to(DEV).contiguous(), trans=trans.to(DEV).contiguous(), shared_beta=True, trans_after_joints=True)
        ndc, _ = eng.project(cams, lbs["verts"], want_yx=False)
        out.append((lbs["verts"], ndc))
    (verts, ndc), (_, ndc_t) = out
    target = (eng.silhouette_forward(dm, ndc_t, S) > 0.5).to(torch.uint8).contiguous()
    return cams, verts, ndc.contiguous(), target


def run(tag, dm, cams, verts, ndc, target, S, K, tie):
    N = ndc.shape[0]
    rs = eng.raster_settings(K=K, tie_rule=tie)
    g = torch.Generator().manual_seed(17 + N + S)
    sil = eng.silhouette_forward(dm, ndc, S, rs)
    st_f = eng.raster_stats(dm, N)
    grad = torch.randn(N, S, S, generator=g).to(DEV)
    d_bwd = eng.silhouette_backward(dm, ndc, S, grad, rs)
    st_b = eng.raster_stats(dm, N)
    scale = ((1.0 + torch.rand(N, generator=g)) / (S * S)).to(DEV)
    loss, d_fused, sil_fused = eng.silhouette_l1_fused(dm, ndc, S, target, eng.image_abs_sum(target), scale, rs, want_sil=True)
    st_l = eng.raster_stats(dm, N)
    keys = ("straddling_faces", "tiles", "unclipped_faces", "tie_pixels")
    save(tag, forward=sil, backward_d_ndc=d_bwd, fused_sil=sil_fused, fused_loss=loss, fused_d_ndc=d_fused,
         stats=np.array([[st[k] for k in keys] for st in (st_f, st_b, st_l)], dtype=np.int64))


def colour(tag, dm, cams, verts, ndc):
    image, p2f = eng.render_colour(dm, cams, verts, (0.2, 0.5, 0.8), verts_ndc=ndc, want_pix_to_face=True)
    save(tag, colour=image, colour_pix_to_face=p2f)


for key in args.models.split(","):
    t = model_io.load_model(os.path.join(REPO, "data", "models", {"stick": "SMILy_STICK", "mouse": "SMILy_Mouse_static_joints"}[key] + ".npz"))
    dm = eng.DeviceModel(t, DEV)
    for S in (int(x) for x in args.sizes.split(",")):
        for N in (int(x) for x in args.images.split(",")):
            cams, verts, ndc, target = scene(t, dm, N, S, 1000 + S + N)
            colour(f"{key}.S{S}.N{N}", dm, cams, verts, ndc)
            for K in (int(x) for x in args.faces_per_pixel.split(",")):
                for tie in ("depth_face_id", "reference_queue"):
                    run(f"{key}.S{S}.N{N}.K{K}.{tie}", dm, cams, verts, ndc, target, S, K, tie)
            torch.cuda.synchronize()
            print(f"{key} S={S} N={N}: {n_saved} arrays so far", flush=True)
    # the mesh through the clipping plane: a few vertices of every image nearer than z_clip, some behind the camera
    S, N = 64, 3
    cams, verts, ndc, target = scene(t, dm, N, S, 77)
    g = torch.Generator().manual_seed(5)
    ndc = ndc.cpu()
    for n in range(N):
        idx = torch.randperm(t.V, generator=g)[:6]
        ndc[n, idx, 2] = torch.tensor([-0.4, 2e-4, -1.5, 1e-5, 4e-4, -0.05])
        ndc[n, idx, :2] *= 0.3
    ndc = ndc.to(DEV).contiguous()
    colour(f"{key}.clip", dm, cams, verts, ndc)
    for tie in ("depth_face_id", "reference_queue"):
        run(f"{key}.clip.K100.{tie}", dm, cams, verts, ndc, target, S, 100, tie)
        run(f"{key}.clip.K4.{tie}", dm, cams, verts, ndc, target, S, 4, tie)
    torch.cuda.synchronize()
print(f"{n_saved} arrays in {args.out} (library: {os.environ.get('SMILFIT_LIB', 'the default build')})")
