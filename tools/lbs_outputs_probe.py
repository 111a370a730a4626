"""Every output of the LBS and projection entry points from seeded inputs, as .npy files: run once per build of the library
(``SMILFIT_LIB`` selects one, smilify_amd/_lib.py) and compare the two directories bit for bit.  For changes to lbs.hip /
project.hip that must not change a single bit (kernels whose instruction stream moved without their arithmetic moving).

    SMILFIT_LIB=smilify_amd/lib/libsmilfit_parent.so python3 tools/lbs_outputs_probe.py --out /tmp/lbs_a
    python3 tools/lbs_outputs_probe.py --out /tmp/lbs_b
    python3 tools/lbs_outputs_probe.py --compare /tmp/lbs_a /tmp/lbs_b

Cases: STICK, the two synthetic models (regressed / static joints), the pose-blend model of tests/golden/lbs_posedirs.npz and
the mouse; B = 5 (the 1024-thread fused kernels, one frame per workgroup) and B = 300 (the 512-thread ones, workgroups walking
several frames); 1 and 3 views; shared and per-frame betas; the translation added before and after the joint regression.
Arrays above four million elements are written as the SHA-256 of their bits.  Everything is compared byte for byte
(tools/probelib.py); a ``fov_img`` that differs (float atomics in an order that varies from run to run) passes within 2e-5 of its
largest entry, and is named.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="directory the .npy files are written to")
ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare two such directories instead of running anything")
ap.add_argument("--models", default="stick,synthetic,synthetic_static,posedirs,mouse")
ap.add_argument("--frames", default="5,300")
ap.add_argument("--views", default="1,3")
args = ap.parse_args()

if args.compare:
    a, b = (probelib.load_arrays(d) for d in args.compare)
    only, changed = probelib.differing(a, b)
    bad, took = [("only in one directory", n + ".npy") for n in only], []
    for n in changed:
        x, y = a[n], b[n]
        if "fov_img" in n:  # float atomics
            err = float(np.abs(x - y).max() / (np.abs(y).max() + 1e-30)) if x.shape == y.shape else np.inf
            (took if err < 2e-5 else bad).append((n + ".npy", err))
        else:
            bad.append((n + ".npy", float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape else "shape"))
    n_fov = sum("fov_img" in n for n in set(a) & set(b))
    print(f"{len(a)} / {len(b)} arrays, {n_fov} of them fov_img (2e-5), the others bit for bit: {len(bad)} differ")
    for x in took:
        print("WITHIN 2e-5", x)
    for x in bad:
        print("DIFFERS", x)
    sys.exit(1 if bad or not a else 0)

import torch  # noqa: E402

from smilify_amd import cameras as cam_mod  # noqa: E402
from smilify_amd import engine as eng  # noqa: E402
from smilify_amd import model_io, synthetic  # noqa: E402

DEV = "cuda:0"
S = 64
BIG = 1 << 22  # elements above which an array is written as the SHA-256 of its bits
os.makedirs(args.out, exist_ok=True)
n_saved = 0


def save(tag, d):
    global n_saved
    for k, v in d.items():
        if isinstance(v, torch.Tensor) and not k.startswith("_"):
            a = v.detach().cpu().numpy()
            if a.size > BIG:  # (the mouse at 300 frames: gigabytes) the digest of the bits stands for the array
                a, k = np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8), k + ".sha256"
            np.save(os.path.join(args.out, f"{tag}.{k}.npy"), a)
            n_saved += 1


def get_tables(key):
    if key == "synthetic":
        return model_io.synthetic_model()
    if key == "synthetic_static":
        return model_io.synthetic_model(static_joints=True, seed=3)
    if key == "posedirs":
        g = np.load(os.path.join(REPO, "tests", "golden", "lbs_posedirs.npz"))
        t = model_io.synthetic_model(seed=int(g["seed"]))
        t.posedirs = g["posedirs"].astype(np.float32)
        return t
    return model_io.load_model(os.path.join(REPO, "data", "models", {"stick": "SMILy_STICK", "mouse": "SMILy_Mouse_static_joints"}[key] + ".npz"))


def pack_rows(d_ndc, g):
    """(N,V,2) floats -> the fused rasteriser's packed rows (x * 2^32 + y, two's complement: `pack_fx2`, csrc/raster_common.h) and their
    per-image factors; image 1 keeps plain floats (factor 0) and the last image a negative factor."""
    N = d_ndc.shape[0]
    scale = (2.0 ** -20) * (1.0 + torch.rand(N, generator=g))
    q = torch.round(d_ndc.cpu() / scale[:, None, None]).to(torch.int32)
    qx, qy = q[..., 0], q[..., 1]
    raw = torch.stack([qy, qx + (qy >> 31)], dim=-1).view(torch.float32)  # low word first
    scale[1 % N] = 0.0
    raw[1 % N] = d_ndc.cpu()[1 % N]
    if N > 2:
        scale[N - 1] = -scale[N - 1]
    return raw.contiguous().to(DEV), scale.to(DEV)


def run_case(key, B, views):
    t = get_tables(key)
    dm = eng.DeviceModel(t, DEV)
    J, V, nB = dm.J, dm.V, dm.nB
    g = torch.Generator().manual_seed(1000 + 7 * B + views)
    R, T = cam_mod.look_at_view_transform(3.0, 10.0, np.linspace(0, 300, views), device=DEV)
    cams = eng.CameraSet(R.contiguous(), T.contiguous(), torch.full((views,), 55.0, device=DEV), None, views, S)
    N = B * views
    theta = (0.25 * torch.randn(B, J, 3, generator=g)).to(DEV)
    trans = (0.1 * torch.randn(B, 3, generator=g)).to(DEV)
    ls = (0.05 * torch.randn(J, 3, generator=g)).to(DEV)
    bt = (0.02 * torch.randn(J, 3, generator=g)).to(DEV)
    betas = {True: (0.4 * torch.randn(nB, generator=g)).to(DEV), False: (0.4 * torch.randn(B, nB, generator=g)).to(DEV)}
    d_ndc = (1e-3 * torch.randn(N, V, 2, generator=g)).to(DEV)
    d_yx = (1e-2 * torch.randn(N, J, 2, generator=g)).to(DEV)
    d_ndc_p, sc_p = pack_rows(d_ndc, g)
    # a handful of cut-edge depth gradients, every entry of a frame on a vertex of its own
    per = 3
    cd = eng.ClipDepth(DEV, N, capacity=max(64, per * N))
    assert per * views <= V
    vid = torch.stack([(torch.arange(per * views) * (V // (per * views)) + b) % V for b in range(B)]).reshape(-1).to(torch.int32)
    cd.vertex[: per * N] = vid.to(DEV)
    cd.dz[: per * N] = (1e-2 * torch.randn(per * N, generator=g)).to(DEV)
    cd.range[:] = torch.stack([per * torch.arange(N), torch.full((N,), per)], dim=1).to(torch.int32).to(DEV)
    cd.range[N // 2, 1] = 0  # (an image without cut faces)
    cd.counter[0] = per * N
    for shared in (True, False):
        for after in (True, False):
            tag = f"{key}.B{B}.v{views}.{'shared' if shared else 'frame'}.{'after' if after else 'before'}"
            kw = dict(trans=trans, logscale=ls, btrans=bt, shared_beta=shared, logscale_shared=True, btrans_shared=True, trans_after_joints=after)
            fwd = eng.lbs_forward(dm, betas[shared], theta, **kw)
            save(tag + ".fwd", fwd)
            for want in (dict(ndc=True, yx=True), dict(ndc=True, yx=False), dict(ndc=False, yx=True)):
                save(tag + f".fwdproj{int(want['ndc'])}{int(want['yx'])}", eng.lbs_forward(dm, betas[shared], theta, project=dict(cams=cams, **want), **kw))
            ndc, yx = eng.project(cams, fwd["verts"])
            ndc2, yx2 = eng.project_verts_and_joints(cams, fwd["verts"], fwd["joints"])
            save(tag + ".project", dict(ndc=ndc, yx=yx, ndc2=ndc2, yx2=yx2))
            # separate route: projection backward (plain and packed rows), the clip-depth term, then the LBS backward
            fov = torch.zeros(N, device=DEV)
            dv, dj = eng.project_backward_verts_and_joints(cams, fwd["verts"], d_ndc, fwd["joints"], d_yx, fov)
            fov_p = torch.zeros(N, device=DEV)
            dv_p, _ = eng.project_backward(cams, fwd["verts"], d_ndc=d_ndc_p, d_fov_img=fov_p, d_ndc_scale=sc_p)
            dj_only, _ = eng.project_backward(cams, fwd["joints"], d_yx=d_yx)
            dv_c = dv.clone()
            eng.clip_depth_backward(cams, cd, dv_c)
            save(tag + ".projbwd", dict(dv=dv, dj=dj, fov_img=fov, dv_packed=dv_p, fov_img_packed=fov_p, dj_only=dj_only, dv_clip=dv_c))
            save(tag + ".bwd", eng.lbs_backward(dm, fwd, dv, dj, need_vshaped=True))
            save(tag + ".bwd_verts_only", eng.lbs_backward(dm, fwd, dv_c, None))
            if eng.lbs_backward_ndc_supported(dm, nB, views):  # the fused route, from the image plane
                for name, up in (("ndc", dict(d_ndc=d_ndc, d_yx=d_yx)), ("ndc_packed", dict(d_ndc=d_ndc_p, d_ndc_scale=sc_p)),
                                 ("ndc_yx_only", dict(d_yx=d_yx)), ("ndc_clip", dict(d_ndc=d_ndc, d_yx=d_yx, clip_depth=cd))):
                    fov_f = torch.zeros(N, device=DEV)
                    out = eng.lbs_backward(dm, fwd, None, None, ndc_upstream=dict(cams=cams, d_fov_img=fov_f, **up))
                    save(tag + ".bwd_" + name, dict(out, fov_img=fov_f))
    torch.cuda.synchronize()


def run_rasteriser_rows():
    """Packed rows as the fused rasteriser itself leaves them (tests/test_gpu_lbs_fused.py), one image with factor 0."""
    t = get_tables("stick")
    N = 80
    f = synthetic.make_problem(t, N, 1, 96, DEV, seed=4, window=N)
    f._refresh_targets()
    dm = f.device_model
    lbs = eng.lbs_forward(dm, f.betas.detach(), f._pose, trans=f.trans.detach().contiguous(), shared_beta=True, trans_after_joints=True)
    cam = f.renderer.cameras
    cams = eng.CameraSet(cam.R.contiguous(), cam.T.contiguous(), f.fov.detach(), None, 1, 96)
    ndc, _ = eng.project(cams, lbs["verts"], want_yx=False)
    scale = torch.full((N,), 3.0 / (96 * 96), device=DEV)
    scale[7] = 0.0
    _, dn_p, _, sc_p = eng.silhouette_l1_fused(dm, ndc, 96, f._sil_dev, f._sil_sum, scale, packed_out=True)
    fov_a, fov_b = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    a = eng.lbs_backward(dm, lbs, None, None, ndc_upstream=dict(cams=cams, d_ndc=dn_p, d_ndc_scale=sc_p, d_fov_img=fov_a))
    dv, _ = eng.project_backward(cams, lbs["verts"], d_ndc=dn_p, d_fov_img=fov_b, d_ndc_scale=sc_p)
    save("raster_rows.fused", dict(a, fov_img=fov_a))
    save("raster_rows.separate", dict(eng.lbs_backward(dm, lbs, dv, None), dv=dv, fov_img=fov_b, ndc=ndc))


for key in args.models.split(","):
    for B in (int(x) for x in args.frames.split(",")):
        for views in (int(x) for x in args.views.split(",")):
            run_case(key, B, views)
            print(f"{key} B={B} views={views}: {n_saved} arrays so far", flush=True)
if "stick" in args.models.split(","):
    run_rasteriser_rows()
print(f"{n_saved} arrays in {args.out} (library: {os.environ.get('SMILFIT_LIB', 'the default build')})")
