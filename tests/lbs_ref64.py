"""Float64 references for the LBS kernels (smilify_amd/csrc/lbs.hip) and the camera projection (project.hip), the case
families both tests/test_lbs_ref64_cpu.py and tests/test_gpu_lbs_float64.py walk, the per-row error metric and its bounds.
Holds no kernels and touches no GPU.

* LBS: ``oracle/lbs_ref.py`` is dtype-generic; ``reference()`` densifies the model tables in the wanted dtype and calls
  ``lbs_ref.smal_forward`` with leaves of that dtype.  The semantics are stated once, in the oracle (reference
  smal_model/smal_torch.py:198-370, batch_lbs.py:31-197).
* Projection: ``oracle/render_ref.project_to_ndc`` / ``project_points_screen`` are dtype-generic as well (formulas in the header
  of project.hip); ``cam_rows`` restates only the ``image % rows`` indexing of the camera tables.
* ``encode_packed`` writes a gradient as the fused rasteriser leaves it (``x * 2^32 + y`` fixed-point words with a per-image
  factor), so that the kernels' decode is checked against integers; ``decode_packed_np`` restates the decode.
* ``row_err``: max over rows of max|got - want| / max|want| within the row.

Bounds
------
``MEASURED[q]`` is the largest ``row_err`` the fp32 CPU oracle shows against the same oracle in float64 over every case family
below (tests/test_lbs_ref64_cpu.py keeps that measurement alive: it asserts oracle32 <= TOL / 16).  The figures move by a few
per cent with the BLAS thread count (summation order of the fp32 matmuls), so each is written rounded UP, with at least a tenth to
spare, to the next of 1, 1.5, 2, 3, 4, 5, 6, 8 x 10^k.  ``TOL[q] = MARGIN[q] * MEASURED[q]``, capped by the bound the older tests use for the same
quantity (2e-5 forward, 3e-4 gradients).  The margin is 16: what a kernel may legitimately do differently from an fp32 torch
evaluation (wave / block reduction orders, fixed-order row sums, float atomics of d_fov_img, expf and 1/x of the device
library).  A margin above 16 (64 at the most) names the long cancelling sum that needs it.
"""
import math

import numpy as np
import torch

from oracle import lbs_ref, render_ref

FWD_CEILING, GRAD_CEILING = 2e-5, 3e-4

# quantity: largest row_err of the fp32 oracle against float64 (as measured with 1 and with 16 threads, the larger one; case that showed it)
MEASURED = {
    # forward
    "verts": 1.5e-6,     # 1.02e-6  pose/synthetic_static-ls1.0-ndc
    "joints": 1e-6,      # 8.5e-7   pose/stick-ls1.0
    "new_J": 1e-6,       # 8.2e-7   pose/stick-ls1.0
    "Rs": 6e-7,          # 5.0e-7   pose/stick-ls0.3
    "A": 1e-6,           # 8.2e-7   pose/synthetic_static-ls1.0-ndc
    "v_shaped": 8e-8,    # 6.5e-8   options/nB_used17-perframe
    "ndc": 1.5e-6,       # 1.00e-6  pose/synthetic_static-ls1.0-ndc
    "ndc_z": 3e-7,       # 2.2e-7   batch/mouse-B257
    "yx": 1e-6,          # 7.0e-7   batch/mouse-B257
    # gradients
    "d_beta": 3e-6,      # 1.85e-6  batch/stick-perframe-B259
    "d_theta": 1.5e-5,   # 1.23e-5  pose/synthetic_static-ls0.3 (the rows at |theta| = pi)
    "d_trans": 8e-6,     # 5.8e-6   batch/stick-B255-v1
    "d_logscale": 2e-6,  # 1.37e-6  options/nB_used6
    "d_btrans": 1.5e-6,  # 9.7e-7   options/nB_used16-perframe
    "d_del_v": 4e-7,     # 3.1e-7   options/del_v-shared-beta
    "d_v_template": 3e-7,  # 2.1e-7 options/v_template
    "d_Rs_in": 5e-7,     # 3.6e-7   options/Rs_in
    "d_joints": 6e-7,    # 4.2e-7   batch/mouse-B257
    "d_fov": 3e-6,       # 1.97e-6  pose/stick-ls0.3-ndc
    "d_pts": 3e-7,       # 1.8e-7   projection/P256
    # projection/near-plane: points 0.05 in front of a camera 3 away, z_view is a difference of numbers 60 times its size
    "ndc_near": 4e-6,    # 3.0e-6
    "ndc_z_near": 1e-7,  # 6.1e-8
    "yx_near": 4e-6,     # 3.1e-6
    "d_pts_near": 8e-6,  # 5.8e-6
    "d_fov_near": 3e-6,  # 1.65e-6
}
MARGIN = {q: 16 for q in MEASURED}
TOL = {q: min(MARGIN[q] * MEASURED[q], FWD_CEILING if not q.startswith("d_") else GRAD_CEILING) for q in MEASURED}


# ----------------------------------------------------------------------------------------------
# metric
# ----------------------------------------------------------------------------------------------
def row_err(got, want, rows):
    """max over rows of max|got - want| / max|want| within the row; ``rows``: the number of rows the tensors are cut into
    (frames for per-frame quantities, 1 for a table shared by all frames).  A row whose reference is exactly zero must be exactly
    zero in ``got``: anything else is an infinite error.  Non-finite values are an infinite error."""
    g = torch.as_tensor(got).detach().cpu().to(torch.float64).reshape(rows, -1)
    w = torch.as_tensor(want).detach().cpu().to(torch.float64).reshape(rows, -1)
    assert g.shape == w.shape, (g.shape, w.shape)
    if not (torch.isfinite(g).all() and torch.isfinite(w).all()):
        return math.inf
    diff, scale = (g - w).abs().amax(1), w.abs().amax(1)
    zero = scale == 0
    if bool((diff[zero] != 0).any()):
        return math.inf
    live = ~zero
    return float((diff[live] / scale[live]).max()) if bool(live.any()) else 0.0


def rows_of(key, case):
    """How many rows ``key`` has in this case (see ``row_err``)."""
    B, fl = case["B"], case["fl"]
    if key == "v_shaped":
        return B if (not fl["shared_beta"] or case["inp"].get("del_v") is not None) else 1
    if key == "d_beta":
        return 1 if fl["shared_beta"] else B
    if key == "d_logscale":
        return 1 if fl["logscale_shared"] else B
    if key == "d_btrans":
        return 1 if fl["btrans_shared"] else B
    if key in ("d_fov", "d_v_template"):
        return 1
    return B


# ----------------------------------------------------------------------------------------------
# model tables and cameras
# ----------------------------------------------------------------------------------------------
def dense_model(t, dtype=torch.float64):
    """Dense tables for ``lbs_ref.smal_forward`` from the product's flat tables, densified in ``dtype`` (the fp32 table entries
    are exact in either)."""
    W = np.zeros((t.V, t.J), np.float64)
    np.add.at(W, (np.repeat(np.arange(t.V), t.skin_idx.shape[1]), t.skin_idx.reshape(-1)), t.skin_w.reshape(-1).astype(np.float64))
    R = np.zeros((t.V, t.J), np.float64)
    for j in range(t.J):
        s, e = t.jreg_rowptr[j], t.jreg_rowptr[j + 1]
        R[t.jreg_col[s:e], j] = t.jreg_val[s:e]
    cv = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    pd = t.posedirs
    return dict(v_template=cv(t.v_template), shapedirs=cv(t.shapedirs), J_regressor=cv(R), weights=cv(W), parents=t.parents.copy(),
                J_static=cv(t.J_static) if t.static_joints else None, posedirs=None if pd is None else cv(pd))


def cam_rows(x, N):
    """Row ``image % rows`` of a camera table for each of N images (CameraSet's indexing)."""
    return x[torch.arange(N) % x.shape[0]]


def look_at(views, dist=3.0, elev=12.0):
    """fp32 (views,3,3), (views,3) look-at cameras on a circle (the values the kernels receive)."""
    R, T = render_ref.look_at_view_transform(dist, elev, torch.linspace(0, 300, views))
    return R.contiguous(), T.contiguous()


def project64(pts, R, T, fov, aspect, views, S, dtype=torch.float64):
    """pts (frames,P,3) -> ndc (N,P,3), yx (N,P,2) with N = frames x views; camera tables of 1, views or N rows."""
    frames, P = pts.shape[0], pts.shape[1]
    N = frames * views
    pe = pts[:, None].expand(-1, views, -1, -1).reshape(N, P, 3)
    Rn, Tn, fn = cam_rows(R.to(dtype), N), cam_rows(T.to(dtype), N), cam_rows(fov, N)
    an = None if aspect is None else cam_rows(aspect.to(dtype), N)
    return render_ref.project_to_ndc(pe, Rn, Tn, fn, an), render_ref.project_points_screen(pe, Rn, Tn, fn, S, an)


# ----------------------------------------------------------------------------------------------
# packed gradients (smil_silhouette_l1_fused, packed_out): x * 2^32 + y, two's complement, times a per-image factor
# ----------------------------------------------------------------------------------------------
def encode_packed(grad, scale):
    """grad (N,P,2) float, scale (N,) float32 >= 0 -> (words (N,P,2) float32 bit patterns, decoded (N,P,2) float64).
    Images with scale > 0 hold ``round(g / scale)`` as one int64 word ``qx * 2^32 + qy`` (a negative qy borrows one from the
    high half); images with scale == 0 keep plain floats.  ``decoded`` is what a correct decode returns: q * scale, or the float."""
    g = np.asarray(grad, np.float64)
    sc = np.asarray(scale, np.float32)
    N = g.shape[0]
    words = np.empty(g.shape[:2], np.int64)
    decoded = np.empty_like(g)
    for n in range(N):
        if sc[n] > 0:
            q = np.rint(g[n] / np.float64(sc[n])).astype(np.int64)
            assert np.abs(q).max() < 2 ** 31
            words[n] = q[:, 0] * (1 << 32) + q[:, 1]
            decoded[n] = q * np.float64(sc[n])
        else:
            f = g[n].astype(np.float32)
            words[n] = f.view(np.uint32).astype(np.int64)[:, 0] | (f.view(np.uint32).astype(np.int64)[:, 1] << 32)
            decoded[n] = f
    return torch.from_numpy(words.view(np.float32).reshape(g.shape).copy()), torch.from_numpy(decoded)


def decode_packed_np(words, scale):
    """numpy restatement of the kernels' decode (project.hip k_project_bwd, lbs.hip k_lbs_bwd_ndc)."""
    w = np.ascontiguousarray(words.numpy()).view(np.int32).reshape(words.shape)  # [..., 0] low half, [..., 1] high half
    sc = np.asarray(scale, np.float32)
    out = np.empty(w.shape, np.float64)
    for n in range(w.shape[0]):
        if sc[n] != 0:
            qy = w[n, :, 0].astype(np.int64)
            qx = w[n, :, 1].astype(np.int64) - (qy >> 31)
            out[n, :, 0], out[n, :, 1] = qx * np.float64(sc[n]), qy * np.float64(sc[n])
            if sc[n] < 0:
                out[n] = 0
        else:
            out[n] = w[n].view(np.float32)
    return out


# ----------------------------------------------------------------------------------------------
# LBS cases
# ----------------------------------------------------------------------------------------------
def probe(shape, k):
    n = int(np.prod(shape))
    return torch.from_numpy(np.cos(0.37 * np.arange(n) * (k + 1) + k).astype(np.float32).reshape(shape))


def edge_theta(J, seed):
    """(8,J,3): one pose edge per frame."""
    g = torch.Generator().manual_seed(seed)
    th = torch.zeros(8, J, 3)
    th[1] = 1e-6 * torch.randn(J, 3, generator=g)
    th[2] = 1e-3 * torch.randn(J, 3, generator=g)
    for i, ang in enumerate((math.pi - 1e-3, math.pi, math.pi + 0.5, 2 * math.pi + 0.1)):
        ax = torch.randn(J, 3, generator=g, dtype=torch.float64)
        th[3 + i] = (ax / ax.norm(dim=1, keepdim=True) * ang).float()
    th[7, :, 0] = 0.7
    return th


def make_case(t, B, seed, views=0, shared_beta=True, logscale_shared=True, btrans_shared=True, trans_after_joints=True,
              propagate_scaling=False, allow_limb_scaling=True, theta=None, theta_scale=0.3, ls_scale=0.05, mask=False, del_v=False,
              v_template=False, Rs_in=False, nB_used=None, up_Rs=False, up_vs=False, logscale=True, btrans=True, S=64, dist=3.0):
    """Inputs (fp32 host tensors, what the kernels receive) and the objective of one call.  ``views`` = 0: the objective is
    sum(verts * probe) + sum(joints * probe) (+ Rs, v_shaped probes); ``views`` > 0: it is taken on the image plane,
    sum(ndc_xy * d_ndc) + sum(yx * d_yx) through ``views`` look-at cameras with per-view fov."""
    g = torch.Generator().manual_seed(seed)
    J, V = t.J, t.V
    nB = t.nB if nB_used is None else nB_used
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = dict(beta=0.4 * rn(*((nB,) if shared_beta else (B, nB))), trans=0.1 * rn(B, 3))
    th = theta_scale * rn(B, J, 3) if theta is None else theta.clone()
    if Rs_in:
        inp["Rs_in"] = lbs_ref.rodrigues(th.double().reshape(-1, 3)).view(B, J, 3, 3).float()
    else:
        inp["theta"] = th
    if logscale:
        inp["ls"] = ls_scale * rn(*((J, 3) if logscale_shared else (B, J, 3)))
    if btrans:
        inp["bt"] = 0.02 * rn(*((J, 3) if btrans_shared else (B, J, 3)))
    if mask:
        inp["theta_mask"] = (torch.rand(J, 3, generator=g) < 0.6).float()
    if del_v:
        inp["del_v"] = 0.01 * rn(B, V, 3)
    if v_template:
        inp["v_template"] = torch.from_numpy(t.v_template) + 0.01 * rn(V, 3)
    fl = dict(shared_beta=shared_beta, logscale_shared=logscale_shared, btrans_shared=btrans_shared, propagate_scaling=propagate_scaling,
              allow_limb_scaling=allow_limb_scaling, trans_after_joints=trans_after_joints)
    up = dict(views=views)
    if views:
        R, T = look_at(views, dist)
        up.update(R=R, T=T, fov=52.0 + torch.arange(views, dtype=torch.float32), S=S,
                  d_ndc=1e-3 * rn(B * views, V, 2), d_yx=1e-2 * rn(B * views, J, 2))
    else:
        up.update(d_verts=probe((B, V, 3), 0), d_joints=probe((B, J, 3), 1))
        if up_Rs:
            up["up_Rs"] = probe((B, J, 3, 3), 2)
        if up_vs:
            up["up_vs"] = probe((B if (not shared_beta or del_v) else 1, V, 3), 3)
    return dict(B=B, inp=inp, fl=fl, up=up, nB_used=nB)


def reference(t, case, dtype=torch.float64):
    """The oracle in ``dtype`` on ``case``: (forward outputs, gradients) as dicts of detached tensors keyed like the kernels'."""
    B, inp, fl, up = case["B"], case["inp"], case["fl"], case["up"]
    m = dense_model(t, dtype)
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in inp.items() if k != "theta_mask"}
    if "v_template" in leaves:
        m["v_template"] = leaves["v_template"]
    ex = lambda x, shared: None if x is None else (x[None].expand(B, *x.shape) if shared else x)  # noqa: E731
    pose = leaves["Rs_in"] if "Rs_in" in leaves else leaves["theta"]
    if "theta_mask" in inp:  # (the kernels return d_theta as the gradient on theta * mask; fit_epilogue applies the mask to it)
        pose = pose * inp["theta_mask"].to(dtype)
        pose.retain_grad()
    after = fl["trans_after_joints"]
    o = lbs_ref.smal_forward(m, ex(leaves["beta"], fl["shared_beta"]), pose, trans=None if after else leaves["trans"],
                             del_v=leaves.get("del_v"), betas_logscale=ex(leaves.get("ls"), fl["logscale_shared"]),
                             betas_trans=ex(leaves.get("bt"), fl["btrans_shared"]), propagate_scaling=fl["propagate_scaling"],
                             allow_limb_scaling=fl["allow_limb_scaling"])
    verts, joints = o["verts"], o["joints"]
    if after:
        verts, joints = verts + leaves["trans"][:, None], joints + leaves["trans"][:, None]
    joints.retain_grad()
    nS = rows_of("v_shaped", case)  # (the oracle returns one row per frame, or the one template when there are no coefficients)
    v_shaped = o["v_shaped"][:nS] if o["v_shaped"].shape[0] >= nS else o["v_shaped"].expand(nS, -1, -1)
    fwd = dict(verts=verts, joints=joints, Rs=o["Rs"], A=o["A"][:, :, :3, :], new_J=o["new_J"], v_shaped=v_shaped)
    fov = None
    if up["views"]:
        fov = up["fov"].to(dtype).clone().requires_grad_()
        ndc, _ = project64(verts, up["R"], up["T"], fov, None, up["views"], up["S"], dtype)
        _, yx = project64(joints, up["R"], up["T"], fov, None, up["views"], up["S"], dtype)
        fwd.update(ndc=ndc[..., :2], ndc_z=ndc[..., 2], yx=yx)
        obj = (ndc[..., :2] * up["d_ndc"].to(dtype)).sum() + (yx * up["d_yx"].to(dtype)).sum()
    else:
        obj = (verts * up["d_verts"].to(dtype)).sum() + (joints * up["d_joints"].to(dtype)).sum()
        if "up_Rs" in up:
            obj = obj + (o["Rs"] * up["up_Rs"].to(dtype)).sum()
        if "up_vs" in up:  # (on the nS rows the call returns, not on the oracle's row per frame)
            obj = obj + (v_shaped * up["up_vs"].to(dtype)).sum()
    obj.backward()
    names = dict(beta="d_beta", theta="d_theta", trans="d_trans", ls="d_logscale", bt="d_btrans", del_v="d_del_v", Rs_in="d_Rs_in",
                 v_template="d_v_template")
    grads = {names[k]: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}
    if case["nB_used"] == 0:
        grads.pop("d_beta")
    if "theta_mask" in inp:
        grads["d_theta"] = pose.grad
    if up["views"]:
        grads["d_joints"] = joints.grad
        grads["d_fov"] = fov.grad
    return {k: v.detach() for k, v in fwd.items()}, {k: v.detach() for k, v in grads.items()}


def get_tables(key, tables=None):
    """``key``: a name the ``tables`` fixture knows, ``nb20`` (twenty shape coefficients) or ``posedirs`` (the pose-blend model of
    tests/golden/lbs_posedirs.npz)."""
    from conftest import GOLDEN
    from smilify_amd import model_io

    if key == "nb20":
        return model_io.synthetic_model(nB=20)
    if key == "posedirs":
        g = np.load(GOLDEN + "/lbs_posedirs.npz")
        t = model_io.synthetic_model(seed=int(g["seed"]))
        t.posedirs = g["posedirs"].astype(np.float32)
        return t
    return tables(key)


def batch_sizes(cus=256):
    """Every B at which lbs.hip changes form: few_frames (64), B <= cus (1024-thread forms), SMALL_BATCH_FRAMES (256: 257 has
    a ragged last block of one live wave, 259 one of three), grid = min(B, cus * per_cu) (blocks loop over frames past 2 cus,
    4 cus)."""
    base = [1, 63, 64, 65, 255, 256, 257, 259, 513, 1027]
    if cus != 256:
        base = [1, 63, 64, 65, cus - 1, cus, cus + 1, cus + 3, 257, 259, 2 * cus + 1, 4 * cus + 3]
    return sorted(set(b for b in base if b > 0))


def lbs_specs(cus=256):
    """The LBS case families: name -> list of (id, model key, make_case keywords)."""
    fam = {"batch": [], "options": [], "pose": []}
    for B in batch_sizes(cus):
        for views in (1, 2):
            fam["batch"].append((f"stick-B{B}-v{views}", "stick", dict(B=B, seed=1000 + B, views=views)))
    fam["batch"] += [(f"mouse-B{B}", "mouse", dict(B=B, seed=2000 + B, views=2)) for B in (3, 257)]
    fam["batch"] += [(f"stick-perframe-B{B}", "stick", dict(B=B, seed=3000 + B, views=2, shared_beta=False)) for B in (65, 259)]
    o = fam["options"]
    for key in ("stick", "synthetic_static"):
        o.append((f"{key}-mask", key, dict(B=7, seed=11, mask=True)))
        o.append((f"{key}-mask-ndc", key, dict(B=7, seed=12, mask=True, views=2)))
    for prop in (False, True):
        o.append((f"perframe-tables-prop{int(prop)}", "stick", dict(B=6, seed=13 + prop, logscale_shared=False, btrans_shared=False,
                                                                   propagate_scaling=prop, ls_scale=0.3)))
        o.append((f"perframe-tables-ndc-prop{int(prop)}", "synthetic", dict(B=6, seed=15 + prop, logscale_shared=False, btrans_shared=False,
                                                                           propagate_scaling=prop, ls_scale=0.3, views=3)))
    o.append(("no-limb-scaling", "stick", dict(B=5, seed=17, allow_limb_scaling=False, ls_scale=0.5)))
    o.append(("Rs_in", "stick", dict(B=5, seed=18, Rs_in=True, shared_beta=False, trans_after_joints=False)))
    o.append(("up_Rs-up_vs", "stick", dict(B=5, seed=19, up_Rs=True, up_vs=True)))
    o.append(("up_Rs-up_vs-perframe", "synthetic_static", dict(B=5, seed=20, up_Rs=True, up_vs=True, shared_beta=False)))
    o.append(("del_v-shared-beta", "stick", dict(B=5, seed=21, del_v=True, up_vs=True)))
    o.append(("v_template", "synthetic", dict(B=5, seed=22, v_template=True, trans_after_joints=False)))
    for n in (0, 3, 4, 6, 7, 8, 9, 16, 17):
        o.append((f"nB_used{n}", "nb20", dict(B=9, seed=30 + n, nB_used=n, views=2)))
        o.append((f"nB_used{n}-perframe", "nb20", dict(B=9, seed=60 + n, nB_used=n, shared_beta=False)))
    o.append(("posedirs-B9", "posedirs", dict(B=9, seed=23, logscale=False, btrans=False, trans_after_joints=False, shared_beta=False)))
    o.append(("posedirs-B9-shared", "posedirs", dict(B=9, seed=24)))
    for key in ("stick", "synthetic_static"):
        for s in (0.3, 1.0):
            fam["pose"].append((f"{key}-ls{s}", key, dict(B=8, seed=40, theta="edge", ls_scale=s, logscale_shared=False)))
            # (limbs scaled by up to e^3 reach past a camera 3 away: the wide scales are seen from 40 away)
            fam["pose"].append((f"{key}-ls{s}-ndc", key, dict(B=8, seed=41, theta="edge", ls_scale=s, views=2, dist=3.0 if s < 1 else 40.0)))
    return fam


def build_case(t, kw):
    kw = dict(kw)
    if isinstance(kw.get("theta"), str):
        kw["theta"] = edge_theta(t.J, kw["seed"])
    return make_case(t, **kw)


# ----------------------------------------------------------------------------------------------
# projection cases
# ----------------------------------------------------------------------------------------------
def projection_specs():
    """(id, keywords): P points (``Pb``: a second set in the same launch), views, fov / aspect tables, which upstream
    gradients exist, accumulate, packed d_ndc, points ``near`` the camera plane."""
    out = []
    for i, P in enumerate((1, 255, 256, 257, 513)):
        out.append((f"P{P}", dict(P=P, views=(1, 3, 32, 3, 1)[i], per_image_fov=bool(i % 2), aspect=bool(i & 2), seed=70 + i)))
    out.append(("two-sets-256-1", dict(P=256, Pb=1, views=3, per_image_fov=True, aspect=True, seed=80)))
    out.append(("two-sets-257-256", dict(P=257, Pb=256, views=1, seed=81)))
    out.append(("two-sets-257-256-v32", dict(P=257, Pb=256, views=32, aspect=True, seed=82)))
    out.append(("ndc-only", dict(P=257, views=3, want=("ndc",), seed=83)))
    out.append(("yx-only", dict(P=257, views=3, want=("yx",), per_image_fov=True, seed=84)))
    out.append(("accumulate", dict(P=257, views=3, accumulate=True, aspect=True, seed=85)))
    out.append(("packed", dict(P=513, views=3, packed=True, want=("ndc",), seed=86)))
    out.append(("packed-yx", dict(P=257, views=32, packed=True, per_image_fov=True, seed=87)))
    out.append(("packed-two-sets", dict(P=257, Pb=256, views=3, packed=True, seed=88)))
    out.append(("near-plane", dict(P=256, views=3, near=True, per_image_fov=True, aspect=True, seed=89)))
    return out


def make_projection_case(P, views, seed, Pb=0, per_image_fov=False, aspect=False, want=("ndc", "yx"), accumulate=False, packed=False,
                         near=False, frames=3, S=128):
    g = torch.Generator().manual_seed(seed)
    N = frames * views
    R, T = look_at(views, dist=3.0, elev=15.0)
    c = dict(P=P, Pb=Pb, views=views, frames=frames, S=S, R=R, T=T, want=want, accumulate=accumulate, near=near)
    c["fov"] = 60.0 + torch.linspace(-3, 3, N if per_image_fov else views)
    c["aspect"] = (1.0 + 0.25 * torch.rand(views, generator=g)) if aspect else None
    sets = []
    for n_pts in (P, Pb) if Pb else (P,):
        pts = 0.5 * torch.randn(frames, n_pts, 3, generator=g)
        if near:  # 0.05 in front of the plane z_view = 0 of view 0:  z_view = pts . R[:, 2] + T_z
            axis = R[0, :, 2]
            pts = pts - ((pts @ axis) + T[0, 2] - 0.05)[..., None] * axis
        s = dict(pts=pts, d_ndc=1e-3 * torch.randn(N, n_pts, 2, generator=g), d_yx=1e-2 * torch.randn(N, n_pts, 2, generator=g))
        if accumulate:
            s["d_pts0"] = torch.randn(frames, n_pts, 3, generator=g)
        sets.append(s)
    if packed:  # (the first set's d_ndc only: the rasteriser writes the vertex gradient)
        sc = torch.full((N,), 2.0 ** -30)
        sc[1::3] = 0.0
        c["d_ndc_scale"] = sc
        sets[0]["d_ndc_words"], dec = encode_packed(sets[0]["d_ndc"].numpy(), sc.numpy())
        sets[0]["d_ndc"] = dec.float()  # what the words decode to (exact in fp32: |q| < 2^24 here)
        assert torch.equal(sets[0]["d_ndc"].double(), dec) and bool((dec[..., 1] < 0).any())
    c["sets"] = sets
    return c


def projection_reference(c, dtype=torch.float64):
    """(forward, gradients) of the projection case in ``dtype``; per set ``ndc``, ``ndc_z``, ``yx``, ``d_pts``; ``d_fov`` once."""
    fov = c["fov"].to(dtype).clone().requires_grad_()
    fwd, leaves, obj = [], [], 0.0
    for i, s in enumerate(c["sets"]):
        pts = s["pts"].to(dtype).clone().requires_grad_()
        ndc, yx = project64(pts, c["R"], c["T"], fov, c["aspect"], c["views"], c["S"], dtype)
        fwd.append(dict(ndc=ndc[..., :2].detach(), ndc_z=ndc[..., 2].detach(), yx=yx.detach()))
        two = len(c["sets"]) == 2  # (a two-set launch: the first set comes with d_ndc, the second with d_yx)
        if (not two and "ndc" in c["want"]) or (two and i == 0):
            obj = obj + (ndc[..., :2] * s["d_ndc"].to(dtype)).sum()
        if (not two and "yx" in c["want"]) or (two and i == 1):
            obj = obj + (yx * s["d_yx"].to(dtype)).sum()
        leaves.append(pts)
    obj.backward()
    grads = [dict(d_pts=p.grad.detach() + (s["d_pts0"].to(dtype) if c["accumulate"] else 0)) for p, s in zip(leaves, c["sets"])]
    return fwd, grads, fov.grad.detach()
