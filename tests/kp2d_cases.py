"""The seeded problems tests/test_kp2d_ref_cpu.py and tests/test_gpu_fit_keypoints2d.py share for the multi-view 2-D keypoint term
(smil_kp2d_fit_eval, ``KeypointFitter2D``).  Holds no kernels and touches no GPU.

Geometry: look-at cameras on a circle, every camera at least 1.5 model lengths from every joint of every frame (asserted here).  ONE
frame (``behind_frame``) is translated past camera 0 - a single joint of a connected model cannot lie behind a camera that keeps that
distance from all the others; ``single_joint_problem`` is the one case that gives the distance up for one joint - so that every joint of it has z_view < -0.1 in view 0 (far from the plane: nothing depends on the
conditioning at z -> znear) and is in front of the other views: its entries are unseen in view 0 and seen in the others.
"""
import torch

import joints_ref
import kp2d_ref
from smilify_amd.cameras import look_at_view_transform

S = 256
F64 = torch.float64
# (model, views, camera tables with a row per image, aspect and principal point, seed) of the problems the GPU file measures row errors
# on; tests/test_kp2d_ref_cpu.py checks each of them first (a seed that fails there is replaced: 102, 106, 108 and 204 were; 116 too)
GPU_PROBLEMS = [("stick", 1, False, True, 101), ("stick", 3, True, True, 112), ("mouse", 1, True, False, 103), ("mouse", 3, False, True, 104),
                ("j65", 3, False, False, 105), ("random_wide", 1, False, True, 126), ("j65", 1, True, True, 107),
                ("random_wide", 3, True, False, 118)]
# (model, frames, views, a row per image, seed): the kernel's block loop - a block holds FRAMES_PER_BLOCK frames of the mouse (four
# waves, JT_MAX_FPB, whose LDS fits below 64 KB) and at most 1024 blocks run, so 4099 frames loop and end in a ragged round - and the
# cap of 64 views
FRAMES_PER_BLOCK = 4
BLOCK_PROBLEMS = [("mouse", 3, 2, True, 201), ("mouse", 4, 2, False, 202), ("mouse", 5, 2, True, 203), ("mouse", 4099, 2, False, 214),
                  ("j3", 2, 64, False, 205), ("j3", 2, 64, True, 206)]
# Problems of the other GPU tests that bound a row error, as keywords of ``problem`` (+ ``key``): both terms in one launch (one seed was
# replaced), the comparison with SMALFitter (S = 64, every joint named once), and ``single_joint_problem``
SINGLE_JOINT_SEED = 301
BOTH_PROBLEMS = [dict(key=k, N=7, views=3, seed=s, per_image=True, with_3d=True) for k, s in (("stick", 36), ("mouse", 46))]
SHIPPED_PROBLEMS = [dict(key=k, N=6, views=v, seed=51 + v, per_image=False, aspect_pp=True, size=64, duplicate=False)
                    for k in ("stick", "mouse") for v in (1, 3)]


def make_cameras(N, views, dist, g, per_image=False, aspect_pp=True):
    """float32 tables of ``views`` rows, or of ``N * views`` rows (a jittered rig per frame; a fov table of ``views`` rows then, so that
    tables of different row counts meet in one call)."""
    k = N * views if per_image else views
    # (evenly spread: no other view looks along view 0's axis)
    azim = (torch.arange(views) * (360.0 / views)).repeat(k // views) + (8.0 * torch.rand(k, generator=g) - 4.0 if per_image else 0.0)
    elev = 12.0 + (6.0 * torch.rand(k, generator=g) - 3.0 if per_image else torch.zeros(k))
    d = dist * (1.0 + (0.1 * torch.rand(k, generator=g) if per_image else torch.zeros(k)))
    R, T = look_at_view_transform(d.numpy(), elev.numpy(), azim.numpy())
    cams = dict(R=R.float().contiguous(), T=T.float().contiguous(), fov=(32.0 + 6.0 * torch.rand(views, generator=g)).float())
    if aspect_pp:
        cams["aspect"] = (1.0 + 0.3 * torch.rand(views, generator=g)).float()
        cams["principal"] = (0.2 * torch.rand(k, 2, generator=g) - 0.1).float()
    return cams


def camera_centres(cams, n_img):
    """(n_img,3) float64: C with C R + T = 0."""
    R, T = (kp2d_ref.pinhole_ref.rows(cams[k], n_img).double() for k in ("R", "T"))
    return -torch.einsum("nj,nij->ni", T, R)


def problem(t, N, views, seed, per_image=False, aspect_pp=True, Jc=None, with_3d=False, noise_px=2.0, shift=0.12, size=S, duplicate=True):
    """float32 parameters, a permuted strict subset of the joints with one duplicate, cameras, and 2-D targets - the projections of the
    model moved and bent a little (a coherent residual: the sums that make d_trans and the root's d_theta do not cancel), plus noise - with:
    a NaN target row, an entry with visibility 0, confidences 0 and NaN, a residual of several hundred pixels, the frame behind camera 0
    and a frame with nothing seen (``dead_frame``).  ``with_3d``: 3-D targets too, visible in the frame that is dead in 2-D."""
    g = torch.Generator().manual_seed(seed)
    J, nB = t.J, t.nB
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    params = dict(betas=0.4 * rn(nB), pose=0.3 * rn(N, J, 3), trans=0.1 * rn(N, 3), log_beta_scales=0.05 * rn(J, 3), betas_trans=0.02 * rn(J, 3))
    mask = (torch.rand(J, 3, generator=g) < 0.8).float()
    Jc = max(3, (2 * J) // 3) if Jc is None else Jc
    canon = torch.randperm(J, generator=g)[:Jc].tolist()
    if duplicate and Jc >= 3:
        canon[-1] = canon[0]
    args = lambda p: tuple(p[k].double() for k in ("betas", "pose", "trans", "log_beta_scales", "betas_trans"))  # noqa: E731
    head = {k: (v[:8] if k in ("pose", "trans") else v) for k, v in params.items()}  # (the model's length: eight frames show it)
    joints = joints_ref.oracle_joints(t, *args(head), mask)
    length = float((joints.amax((0, 1)) - joints.amin((0, 1))).max())
    dist = 3.0 * max(length, 0.5)
    cams = make_cameras(N, views, dist, g, per_image, aspect_pp)
    behind_frame, dead_frame = (4, 2) if N >= 6 else (None, None)
    if behind_frame is not None:  # past camera 0 of that frame, on its axis
        c0 = camera_centres(cams, N * views)[behind_frame * views]
        params["trans"][behind_frame] = (2.0 * c0).float()
    joints = joints_ref.oracle_joints(t, *args(params), mask)
    centres = camera_centres(cams, N * views).reshape(N, views, 1, 3)
    gap = (joints[:, None] - centres).norm(dim=-1).min().item()
    assert gap >= 1.5 * length, f"a camera is {gap / length:.2f} model lengths from a joint"
    yx, z = kp2d_ref.project(joints[:, canon], cams, size, views)
    if behind_frame is not None:
        assert bool((z[behind_frame, 0] < -0.1).all()) and bool((z[behind_frame, 1:] > 0.5 * length).all())
        zz = z.clone()
        zz[behind_frame, 0] = float("inf")
        assert bool((zz > 0.5 * length).all())
    # (one offset common to all frames plus a smaller one per frame: the sums over frames that make the shared tables' gradients do not
    # cancel either)
    moved = dict(params, trans=params["trans"] + shift * length * (rn(1, 3) + 0.3 * rn(N, 3)), pose=params["pose"] + 0.05 * (rn(1, J, 3) + 0.3 * rn(N, J, 3)))
    joints_moved = joints_ref.oracle_joints(t, *args(moved), mask)
    yx_t, _ = kp2d_ref.project(joints_moved[:, canon], cams, size, views)
    target = (yx_t + noise_px * (size / S) * rn(N, views, Jc, 2).double()).float()
    vis = torch.ones(N, views, Jc, dtype=torch.uint8)
    conf = (0.5 + torch.rand(N, views, Jc, generator=g)).float()
    target[0, 0, 1] = float("nan")          # a NaN target row
    target[1, views - 1, 0, 1] = float("inf")
    vis[0, 0, 0] = 0                          # an entry with visibility 0
    conf[1, 0, 1] = 0.0
    conf[1, 0, 2] = float("nan")
    target[N - 1, views - 1, Jc - 2] += 350.0 * size / S  # far beyond any sigma
    if dead_frame is not None:
        target[dead_frame, :, :, 0] = float("nan")  # (through the targets: the frame is dead without a visibility table too)
    wj = (0.5 + torch.rand(Jc, generator=g)).double()
    wj[Jc // 2] = 0.0
    out = dict(params=params, mask=mask, canon=canon, cams=cams, S=size, target=target, vis=vis, conf=conf, wj=wj, length=length,
               behind_frame=behind_frame, dead_frame=dead_frame, views=views, N=N)
    if with_3d:
        target3d = (joints_moved[:, canon] + 0.02 * length * rn(N, Jc, 3).double()).float()  # (the same coherent offset, in 3-D)
        target3d[0, 1] = 0.0
        target3d[1, 0, 2] = float("nan")
        vis3d = torch.ones(N, Jc, dtype=torch.uint8)
        vis3d[0, 0] = 0
        out.update(target3d=target3d, vis3d=vis3d)
    return out


def single_joint_problem(t, seed, views=3, N=3):
    """ONE joint behind ONE camera: the three-joint tube with its last joint carried past camera 1 by a large ``betas_trans`` row (the
    joint's position is affine in its own row: the row is solved for from three unit probes), z_view < -0.1 there in every frame and
    well in front of the other views; the other two joints keep 1.5 model lengths from every camera.  Within (frame, view 1) seen and
    unseen depth entries stand side by side.  Small poses, so that the shared row carries the joint past the camera in every frame."""
    g = torch.Generator().manual_seed(seed)
    J, nB = t.J, t.nB
    assert J == 3
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    params = dict(betas=0.4 * rn(nB), pose=0.05 * rn(N, J, 3), trans=0.05 * rn(N, 3), log_beta_scales=0.05 * rn(J, 3), betas_trans=torch.zeros(J, 3))
    mask = torch.ones(J, 3)
    args = lambda p: tuple(p[k].double() for k in ("betas", "pose", "trans", "log_beta_scales", "betas_trans"))  # noqa: E731
    base = joints_ref.oracle_joints(t, *args(params), mask)
    length = float((base.amax((0, 1)) - base.amin((0, 1))).max())
    cams = make_cameras(N, views, 3.0 * max(length, 0.5), g, False, True)
    c1 = camera_centres(cams, views)[1]
    cols = []
    for k in range(3):
        probe = dict(params, betas_trans=params["betas_trans"].clone())
        probe["betas_trans"][2, k] = 1.0
        cols.append(joints_ref.oracle_joints(t, *args(probe), mask)[0, 2] - base[0, 2])
    A = torch.stack(cols, 1)
    params["betas_trans"][2] = torch.linalg.solve(A, 1.3 * c1 - base[0, 2]).float()
    joints = joints_ref.oracle_joints(t, *args(params), mask)
    canon = [2, 0, 1]
    yx, z = kp2d_ref.project(joints[:, canon], cams, S, views)
    assert bool((z[:, 1, 0] < -0.1).all()) and bool((z[:, 1, 1:] > 0.5 * length).all()) and bool((z[:, [0, 2]] > 0.5 * length).all())
    centres = camera_centres(cams, N * views).reshape(N, views, 1, 3)
    assert (joints[:, None, :2] - centres).norm(dim=-1).min().item() >= 1.5 * length
    moved = dict(params, trans=params["trans"] + 0.12 * length * (rn(1, 3) + 0.3 * rn(N, 3)), pose=params["pose"] + 0.05 * (rn(1, J, 3) + 0.3 * rn(N, J, 3)))
    yx_t, _ = kp2d_ref.project(joints_ref.oracle_joints(t, *args(moved), mask)[:, canon], cams, S, views)
    target = (yx_t + 2.0 * rn(N, views, 3, 2).double()).float()
    return dict(params=params, mask=mask, canon=canon, cams=cams, S=S, target=target, vis=torch.ones(N, views, 3, dtype=torch.uint8),
                conf=(0.5 + torch.rand(N, views, 3, generator=g)).float(), wj=(0.5 + torch.rand(3, generator=g)).double(), length=length,
                behind_frame=None, dead_frame=None, views=views, N=N)


def reference(t, p, w_k2d, sigma_px, window, weights=True, w_k3d=0.0, sigma=0.0, dtype=F64):
    """``kp2d_ref.fit_eval`` of a problem; ``weights`` False: no visibility, confidences and joint weights (the NULL paths)."""
    return kp2d_ref.fit_eval(t, p["params"], p["mask"], p["cams"], p["S"], p["target"], p["vis"] if weights else None,
                             p["conf"] if weights else None, p["wj"] if weights else None, p["canon"], w_k2d, sigma_px, window, w_k3d=w_k3d,
                             robust_scale=sigma, target3d=p.get("target3d") if w_k3d > 0 else None,
                             visibility3d=p.get("vis3d") if (w_k3d > 0 and weights) else None, dtype=dtype)
