"""Benchmark of the SMIL fitting inner loop on MI355X.

One "step" = one fit iteration (reference optimize_to_joints.py:147-175): LBS -> projection -> soft
silhouette -> six loss terms -> backward -> Adam, over the whole synthetic batch held by a rank.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full                    (everything below, not just the headline)
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR       (also the last step's outputs as DIR/<name>.npy)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...          (no launcher: starts the line above as a child process and relays it)

Default workload: cfg2b (STICK, 4096 frames x 1 view @256^2), the configuration BASELINE.json's north-star
roofline target is stated on; ``--workload`` selects the other BASELINE configs.

Rank 0 prints ONE JSON line (contract in the task statement) with ``roofline`` (dominant kernel = the fused
tile rasteriser, timed live with HIP events on its launch stream, inside the timed steps).  A plain run does nothing
else: set up, warm up, time ``--steps`` steps, print.  ``--full`` adds what the headline does not need: the
self-check against the CPU oracle (``parity_check``), ``cpu_baseline`` (the CPU oracle timed on the host cores on a
bounded sample of the same workload, rank 0 at N=1 only) and ``other_workloads`` (default workload, one GPU).
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

WORKLOADS = {
    # BASELINE.json configs[1]: "SMIL_OmniAnt.pkl, batch=512 synthetic frames, 1 view, 256x256, 1xMI355X"
    # (SMILy_STICK stands in for the absent OmniAnt pickle)
    "cfg2": dict(model="SMILy_STICK", frames=512, views=1, S=256, radius=2.7, name="cfg2: STICK (OmniAnt stand-in) B=512 x 1 view @256^2"),
    "cfg2b": dict(model="SMILy_STICK", frames=4096, views=1, S=256, radius=2.7, name="cfg2b: STICK (OmniAnt stand-in) B=4096 x 1 view @256^2"),
    "cfg3": dict(model="SMILy_Mouse_static_joints", frames=256, views=18, S=256, radius=4.0,
                 name="cfg3: Mouse_static_joints (Falkner stand-in) B=256 x 18 views @256^2"),
    "cfg4": dict(model="SMILy_STICK", frames=256, views=4, S=512, radius=2.7, name="cfg4: STICK B=256/GPU x 4 views @512^2"),
    # BASELINE.json configs[4] is 8192 frames/GPU of this shape (weak scaling); cfg5s is the same shape at 128 frames
    "cfg5": dict(model="SMILy_Mouse_static_joints", frames=8192, views=18, S=512, radius=4.0,
                 name="cfg5: Mouse_static_joints (Falkner stand-in) 8192 frames/GPU x 18 views @512^2"),
    "cfg5s": dict(model="SMILy_Mouse_static_joints", frames=128, views=18, S=512, radius=4.0,
                  name="cfg5s: Mouse_static_joints 128 frames x 18 views @512^2 (cfg5 shape, reduced frame count)"),
    "tiny": dict(model="SMILy_STICK", frames=16, views=1, S=128, radius=2.7, name="tiny: STICK B=16 @128^2"),
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
HBM_ACHIEVABLE_GBS = 6290.0  # same guide: measured float4 copy
PEAK_CLOCK_HZ = 2.4e9
N_SIMD = 1024  # 256 CUs x 4 SIMD-32: one wave64 VALU instruction occupies a SIMD's pipe for 2 cycles
TRAFFIC_FILES = ("r6_traffic.json", "r5_traffic.json", "r4_traffic.json", "r3_traffic.json", "r2_traffic.json")  # PMC counts per launch (tools/pmc_traffic.sh); the newest that exists is used
PARITY_TOL = 1e-4  # north star: fp32 losses within 1e-4 relative of the reference algorithm (here: its CPU oracle)


def algorithmic_bytes(V, J, S, views):
    """per (frame,view) render fwd + loss fwd + render bwd, and per frame LBS fwd+bwd+Adam."""
    per_view = 36 * V + 20 * S * S + 28 * J + 56
    per_frame = 24 * V + 240 * J + 120
    return per_view, per_frame


def cpu_sample(fitter, n_frames):
    """Host copies of the first ``n_frames`` frames of the workload (parameters as initialised, targets, cameras):
    taken before the first GPU step so that the CPU oracle is timed on the workload's own inputs."""
    views = fitter.views
    c = lambda t: t.detach().float().cpu().clone()  # noqa: E731
    n_img = n_frames * views
    return dict(
        params=dict(betas=c(fitter.betas), log_beta_scales=c(fitter.log_beta_scales[:n_frames]), betas_trans=c(fitter.betas_trans[:n_frames]),
                    global_rotation=c(fitter.global_rotation[:n_frames]), trans=c(fitter.trans[:n_frames]),
                    joint_rotations=c(fitter.joint_rotations[:n_frames]), fov=c(fitter.fov)),
        sil=c(fitter.sil_imgs[:n_img]), joints=c(fitter.target_joints[:n_img]), visibility=fitter.target_visibility[:n_img].cpu().clone(),
        R=c(fitter.renderer.cameras.R), T=c(fitter.renderer.cameras.T), mean_betas=c(fitter.mean_betas), betas_prec=c(fitter.betas_prec),
        n_frames=n_frames, views=views)


def cpu_baseline(tables, wl, sample, window, frames_per_fit_iter, iters=3):
    """Time the CPU oracle (a port of the reference algorithm) on a bounded sample of the same workload: one warm-up
    iteration, then ``iters`` timed fit iterations (forward + backward of the full loss + Adam step), host cores only."""
    import numpy as np

    from oracle import fitter_ref, render_ref
    from smilify_amd import synthetic

    n_frames, views, S = sample["n_frames"], sample["views"], wl["S"]
    model = dict(v_template=torch.from_numpy(tables.v_template), shapedirs=torch.from_numpy(tables.shapedirs),
                 J_regressor=torch.from_numpy(tables.dense_J_regressor()), weights=torch.from_numpy(tables.dense_weights()),
                 parents=tables.parents, faces=torch.from_numpy(tables.faces.astype(np.int64)),
                 J_static=torch.from_numpy(tables.J_static) if tables.static_joints else None, posedirs=None)
    params = {k: v.clone() for k, v in sample["params"].items()}
    for k in ("betas", "log_beta_scales", "global_rotation", "trans", "joint_rotations", "fov"):
        params[k].requires_grad_()
    opt = torch.optim.Adam([p for p in params.values() if p.requires_grad], lr=synthetic.STAGE1_LR, betas=(0.5, 0.999))
    windows = [list(range(s0, min(n_frames, s0 + window))) for s0 in range(0, n_frames, window)]

    def iteration():
        opt.zero_grad()
        total = 0.0
        for v in range(views):  # the oracle renderer takes one camera per image: one pass per view
            tg = dict(sil=sample["sil"][v::views], joints=sample["joints"][v::views], visibility=sample["visibility"][v::views])
            cams = dict(R=sample["R"][v:v + 1], T=sample["T"][v:v + 1])
            for br in windows:
                loss, _, _ = fitter_ref.fit_losses(model, params, br, synthetic.STAGE1_WEIGHTS, tg, cams, S, sample["mean_betas"],
                                                   sample["betas_prec"])
                total = total + loss
        jl, gl, tl = fitter_ref.temporal(params, synthetic.STAGE1_TEMPORAL)
        (total + jl + gl + tl).backward()
        opt.step()
        return float(total)

    iteration()  # warm-up (thread pools, page faults, the oracle's shared object)
    t0 = time.perf_counter()
    for _ in range(iters):
        iteration()
    dt = (time.perf_counter() - t0) / iters
    try:
        cores = min(render_ref.num_threads(), len(os.sched_getaffinity(0)))
    except AttributeError:
        cores = render_ref.num_threads()
    # in the headline's unit: fit iterations over `frames_per_fit_iter` frames per second, from the sample's frame rate (the oracle's
    # cost is linear in the number of frames: every frame is its own LBS + naive raster)
    return dict(value=(n_frames / dt) / frames_per_fit_iter, unit=f"fit-iters/s ({frames_per_fit_iter}-frame iterations, from the sample's frame rate)",
                frame_iters_per_s=n_frames / dt, cores=cores, omp_threads=render_ref.num_threads(),
                torch_threads=torch.get_num_threads(), kind="port", iterations_timed=iters, warmup_iterations=1, s_per_iteration=dt,
                sample=f"first {n_frames} frames x {views} view(s) @ {S}^2 of the same workload (same parameters, targets and cameras), "
                       f"{iters} timed fit iterations after 1 warm-up (oracle: torch-CPU LBS/losses + OpenMP C naive rasteriser), "
                       f"{dt:.2f} s per iteration")


def parity_oracle(tables, wl, sample):
    """Loss of ONE window holding the sample's frames (all views, no temporal term) and its gradients w.r.t. the per-frame
    parameters, from the CPU oracle: what ``SMALFitter.forward`` of the reference returns for that window
    (fitter.py:292-335).  The oracle renderer takes one camera per image: evaluated per view, image means averaged."""
    import numpy as np

    from oracle import fitter_ref
    from smilify_amd import synthetic

    n_frames, views, S = sample["n_frames"], sample["views"], wl["S"]
    model = dict(v_template=torch.from_numpy(tables.v_template), shapedirs=torch.from_numpy(tables.shapedirs),
                 J_regressor=torch.from_numpy(tables.dense_J_regressor()), weights=torch.from_numpy(tables.dense_weights()),
                 parents=tables.parents, faces=torch.from_numpy(tables.faces.astype(np.int64)),
                 J_static=torch.from_numpy(tables.J_static) if tables.static_joints else None, posedirs=None)
    params = {k: v.clone() for k, v in sample["params"].items()}
    for k in ("global_rotation", "trans", "joint_rotations"):
        params[k].requires_grad_()
    total = 0.0
    for v in range(views):
        tg = dict(sil=sample["sil"][v::views], joints=sample["joints"][v::views], visibility=sample["visibility"][v::views])
        loss, _, _ = fitter_ref.fit_losses(model, params, range(n_frames), synthetic.STAGE1_WEIGHTS, tg,
                                           dict(R=sample["R"][v:v + 1], T=sample["T"][v:v + 1]), S, sample["mean_betas"], sample["betas_prec"])
        total = total + loss / views
    total.backward()
    grad = torch.cat([params["global_rotation"].grad.reshape(n_frames, -1), params["joint_rotations"].grad.reshape(n_frames, -1),
                      params["trans"].grad.reshape(n_frames, -1)], 1)
    return float(total.detach()), grad


def parity_check(fitter, tables, wl, sample, window):
    """The run the driver times checks itself (outside the timed region): (1) the six loss terms of the sample's frames as
    one window, HIP path against the CPU oracle on identical inputs; (2) the gradient of the per-frame parameters of those
    frames taken from an evaluation of the WHOLE batch (the launch size the bench times: packed-atomic gradient path, all
    tiles in flight), against the oracle's autograd.  Frames are independent given the shared parameters, so the rows of
    the first window of a batch evaluated in windows of ``n`` frames are the gradients of that window's loss."""
    from smilify_amd import synthetic

    n = sample["n_frames"]
    want, g_ref = parity_oracle(tables, wl, sample)
    objs, _ = fitter._loss_and_grads(list(range(n)), synthetic.STAGE1_WEIGHTS, 0.0)
    got = float(objs[:6].sum().item())
    _, grads = fitter._loss_and_grads(None, synthetic.STAGE1_WEIGHTS, 0.0, window=n)
    g = torch.cat([grads["pose"][:n].reshape(n, -1), grads["trans"][:n].reshape(n, -1)], 1).float().cpu()
    rel = abs(got - want) / max(abs(want), 1e-30)
    grad_rel = float((g - g_ref).norm() / g_ref.norm().clamp_min(1e-30))
    return {"frames": n, "gpu": got, "oracle": want, "rel": rel, "tol": PARITY_TOL, "grad_rel_l2": grad_rel, "grad_tol": 1e-2,
            "ok": bool(rel <= PARITY_TOL and grad_rel <= 1e-2),
            "note": "loss: six terms of the first frames as one window, HIP vs CPU oracle; gradient: d/d(pose, trans) of those frames "
                    "out of a whole-batch evaluation (the timed launch size) vs the oracle's autograd (tolerance as tests/: the "
                    "(depth, face id) tie rule, DESIGN.md section 4)"}


def time_other_workload(key, dev, steps=5, warmup=3, frames=0, graph=False, tie_rule=None):
    """One of the other BASELINE configurations, timed AFTER the headline region and outside it (rank 0, one GPU): the same fit
    iteration on that configuration's own synthetic problem.  Returns ms per step, the tile kernel's average launch time from
    HIP events, and the roofline fraction by the same definition as the headline (algorithmic bytes per launch / kernel time)."""
    from smilify_amd import engine, model_io, synthetic

    wl = WORKLOADS[key]
    tables = model_io.load_model(os.path.join(REPO, "data", "models", wl["model"] + ".npz"))
    n_frames, views, S = (frames or wl["frames"]), wl["views"], wl["S"]
    fitter = synthetic.make_problem(tables, n_frames, views, S, dev, radius=wl["radius"], seed=1234, window=10)
    if tie_rule:
        fitter.renderer.raster_settings = engine.raster_settings(tie_rule=tie_rule)
    fitter.begin_stage(synthetic.STAGE1_LR, fov_lr=1.0)
    step = fitter.fit_step_graph if graph else fitter.fit_step
    for _ in range(warmup):
        step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL)
    torch.cuda.synchronize()
    engine.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kern_ms, kern_n = engine.profile_read()
    engine.profile_enable(False)
    per_view, _ = algorithmic_bytes(tables.V, tables.J, S, views)
    n_img = n_frames * views
    launches_per_step = max(1, round(kern_n / max(steps, 1)))
    kern_avg = kern_ms / max(kern_n, 1)
    achieved = (n_img / launches_per_step * per_view) / (kern_avg * 1e-3) / 1e9 if kern_n else 0.0
    out = {"workload": wl["name"] + (f" [--frames {n_frames}]" if frames else "") + (f" [tie_rule {tie_rule}]" if tie_rule else ""), "frames": n_frames, "images": n_img, "steps": steps,
           "ms_per_step": 1000.0 * dt / steps, "frame_iters_per_s": n_frames / (dt / steps), "kernel_ms": kern_avg if kern_n else None,
           "launches_per_step": launches_per_step, "frac": achieved / HBM_PEAK_GBS if kern_n else None}
    del fitter
    torch.cuda.empty_cache()
    return out


def time_reference_loop(key, dev, epochs=20, warmup=3, fit_step_ms=None):
    """The reference's UNCHANGED driver body (optimize_to_joints.py:117-127,147-175) on one of the workloads: torch.optim.Adam over
    named_parameters with fov in its own group, per WINDOW_SIZE window ``model(batch_range, weights, stage_id)``, ``get_temporal``, one
    ``backward()``, ``optimizer.step()``, and the loss read back once per epoch as the reference's progress line does.  This is the
    boundary a user of the reference calls; ``fit_step`` (the headline) is the fused extension behind it."""
    from smilify_amd import model_io, synthetic

    wl = WORKLOADS[key]
    tables = model_io.load_model(os.path.join(REPO, "data", "models", wl["model"] + ".npz"))
    n, window = wl["frames"], 10
    model = synthetic.make_problem(tables, n, wl["views"], wl["S"], dev, radius=wl["radius"], seed=1234, window=window)
    weights, w_temp, lr = synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL, synthetic.STAGE1_LR
    optimizer = torch.optim.Adam([{"params": [p for name, p in model.named_parameters() if name != "fov"], "lr": lr},
                                  {"params": [model.fov], "lr": 1}], lr=lr, betas=(0.5, 0.999))

    def epoch():
        acc_loss = 0
        optimizer.zero_grad()
        for j in range(0, n, window):
            loss, _ = model(list(range(j, min(n, j + window))), weights, 1)
            acc_loss += loss.mean()
        joint_loss, global_loss, trans_loss = model.get_temporal(w_temp)
        desc = "{:.2f} ({}, {}, {})".format(acc_loss.data, joint_loss.data, global_loss.data, trans_loss.data)  # (the reference's progress line: a host read per epoch)
        acc_loss = acc_loss + joint_loss + global_loss + trans_loss
        acc_loss.backward()
        optimizer.step()
        return desc

    for _ in range(warmup):
        epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        epoch()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / epochs
    served = model._epoch["served"] if model._epoch else 0
    out = {"workload": wl["name"] + " [reference driver loop: forward per window of 10 + get_temporal + backward + torch.optim.Adam]",
           "frames": n, "windows": (n + window - 1) // window, "epochs": epochs, "ms_per_epoch": ms, "frame_iters_per_s": n / (ms * 1e-3),
           "windows_served_from_one_evaluation": served, "fit_step_ms": fit_step_ms,
           "ratio_to_fit_step": (ms / fit_step_ms) if fit_step_ms else None}
    del model, optimizer
    torch.cuda.empty_cache()
    return out


def time_smal_call(key, dev, frames=4096, reps=30):
    """The drop-in ``SMAL`` module on its own, as the reference's neural caller uses it (one beta row per frame,
    smil_image_regressor.py:2663): ``SMAL.__call__`` forward + ``backward()`` through verts and joints at ``frames`` frames.  Bytes by
    SURVEY.md 8(d)'s LBS figure without the Adam part (24V + 240J per frame: every tensor the API exposes written / read once)."""
    from smilify_amd import model_io
    from smilify_amd.smal_torch import SMAL

    wl = WORKLOADS[key]
    t = model_io.load_model(os.path.join(REPO, "data", "models", wl["model"] + ".npz"))
    smal = SMAL(dev, tables=t)
    g = torch.Generator().manual_seed(1)
    beta = (0.5 * torch.randn(frames, t.nB, generator=g)).to(dev).requires_grad_()
    theta = (0.15 * torch.randn(frames, t.J, 3, generator=g)).to(dev).requires_grad_()
    trans = (0.05 * torch.randn(frames, 3, generator=g)).to(dev).requires_grad_()
    ls = (0.05 * torch.randn(frames, t.J, 3, generator=g)).to(dev).requires_grad_()
    gv = torch.randn(frames, t.V, 3, generator=g).to(dev)
    gj = torch.randn(frames, t.J, 3, generator=g).to(dev)

    def call():
        verts, joints, _, _ = smal(beta, theta, trans=trans, betas_logscale=ls)
        torch.autograd.backward([verts, joints], [gv, gj])
        for p_ in (beta, theta, trans, ls):
            p_.grad = None

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / reps
    alg = frames * (24 * t.V + 240 * t.J)
    out = {"workload": f"SMAL.__call__ forward + backward, {wl['model']}, {frames} frames, one beta row per frame", "frames": frames, "ms_per_call": ms,
           "frames_per_s": frames / (ms * 1e-3), "algorithmic_bytes": alg, "frac": (alg / (ms * 1e-3) / 1e9) / HBM_PEAK_GBS,
           "memory_growth_bytes": int(torch.cuda.memory_allocated() - mem0)}
    del smal, beta, theta, trans, ls, gv, gj
    torch.cuda.empty_cache()
    return out


DUMP_MAX_BYTES = 64 * 10 ** 6
DUMP_PARAMS = ("betas", "log_beta_scales", "betas_trans", "global_rotation", "joint_rotations", "trans", "fov")


def dump_outputs(out_dir, objs, fitter):
    """What a caller of ``fit_step`` holds after the last timed step: the loss terms it returned (``objs``) and the parameters
    its Adam step left (this rank's frames), as float32 ``out_dir/<name>.npy``.  Arrays over an even share of DUMP_MAX_BYTES keep
    a fixed sample of their rows (seeded by name and shape only, so that two builds keep the same rows)."""
    import zlib

    import numpy as np

    arrays = {"objs": objs}
    arrays.update({n: getattr(fitter, n) for n in DUMP_PARAMS})
    arrays = {n: t.detach().float().cpu().numpy() for n, t in arrays.items()}
    share = DUMP_MAX_BYTES // len(arrays) - 4096  # (room for the .npy headers)
    os.makedirs(out_dir, exist_ok=True)
    for n, a in arrays.items():
        if a.nbytes > share:
            keep = max(1, share // (a.nbytes // a.shape[0]))
            rng = np.random.default_rng(zlib.crc32(f"{n}{a.shape}".encode()))
            a = a[np.sort(rng.choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, n + ".npy"), np.ascontiguousarray(a))


def relaunch_multi_gpu(args) -> int:
    """``python bench.py --gpus N`` without a launcher: start one rank per GPU with torch.distributed.run as a CHILD
    process (never exec: nothing here has touched the GPU yet, and it stays that way in this process), relay its output
    and return its exit code."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env)
    return proc.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="cfg2b", choices=sorted(WORKLOADS))
    ap.add_argument("--frames", type=int, default=0, help="override the workload's frames per GPU (tests, rehearsals)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the self-check against the CPU oracle, the CPU baseline and the short runs of the other "
                         "BASELINE configurations (--cpu-frames, --no-parity and --no-others apply to this mode only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (its loss terms, the parameters after its Adam "
                         "step) as DIR/<name>.npy")
    ap.add_argument("--cpu-frames", type=int, default=-1, help="frames of the CPU baseline sample (0 = skip; default: about 8 images)")
    ap.add_argument("--no-parity", action="store_true", help="skip the self-check against the CPU oracle (it needs --cpu-frames > 0)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend; gloo + --share-gpu rehearses the multi-rank path on a 1-GPU box")
    ap.add_argument("--share-gpu", action="store_true", help="every rank uses cuda:0 (rehearsal only; never for reported numbers)")
    ap.add_argument("--tie-rule", default="depth_face_id", choices=["depth_face_id", "reference_queue"],
                    help="which faces a truncated pixel keeps among equal depths at its K-th place (DESIGN.md section 4.2, item 1); the "
                         "reported headline uses the default")
    ap.add_argument("--no-others", action="store_true",
                    help="skip the short runs of the other BASELINE configurations behind the headline region (default workload, one GPU)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(relaunch_multi_gpu(args))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist

    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    from smilify_amd import _lib

    # fresh checkout: rank 0 alone decides and builds (the Makefile links to a temporary name and renames it), every
    # rank then meets at the same barrier, and the library is loaded only behind it
    if rank == 0 and not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    if world > 1:
        dist.barrier()
    from smilify_amd import engine, model_io, optimize, synthetic

    wl = WORKLOADS[args.workload]
    tables = model_io.load_model(os.path.join(REPO, "data", "models", wl["model"] + ".npz"))
    frames, views, S = (args.frames or wl["frames"]), wl["views"], wl["S"]
    window = 10  # reference config.WINDOW_SIZE
    # weak scaling: every rank holds `frames` frames of one long sequence (shards aligned to windows); all ranks draw the
    # sequence from the same seed and keep their own slice
    fitter = synthetic.make_problem(tables, frames, views, S, dev, radius=wl["radius"], seed=1234, window=window,
                                    frame0=rank * frames, n_frames_total=world * frames)
    if args.tie_rule != "depth_face_id":
        fitter.renderer.raster_settings = engine.raster_settings(tie_rule=args.tie_rule)
    n_cpu = 0
    if args.full and rank == 0 and world == 1 and args.cpu_frames != 0:
        n_cpu = min(frames, args.cpu_frames if args.cpu_frames > 0 else max(1, 8 // views))
        sample = cpu_sample(fitter, n_cpu)
    parity = cpu_base = None
    if n_cpu and not args.no_parity:  # before the first step, outside the timed region
        parity = parity_check(fitter, tables, wl, sample, window)
    if n_cpu:  # the CPU oracle first (host cores only), so that everything the GPU does in this run is one contiguous stretch at the end
        cpu_base = cpu_baseline(tables, wl, sample, window, frames)
    fitter.begin_stage(synthetic.STAGE1_LR, fov_lr=1.0)
    staged = args.backend == "gloo"  # gloo: stage the (tiny) collective payloads through host memory
    hook = (lambda block: optimize.allreduce_block(block, host_staged=staged)) if world > 1 else None

    def step():
        halo = None
        if world > 1:  # temporal halo: each shard's first / last parameter row, posted now and waited for in front of the epilogue kernel
            first, last = fitter.boundary_rows()
            halo = optimize.post_halos(first, last, rank, world, host_staged=staged)
        return fitter.fit_step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL, window=window, halo=halo, shared_grad_hook=hook)

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    engine.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        objs = step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kern_ms, kern_n = engine.profile_read()
    engine.profile_enable(False)
    t = torch.tensor([dt], device="cpu" if staged else dev)
    rank_ms = [1000.0 * dt / args.steps]
    if world > 1:
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        rank_ms = [1000.0 * float(x.item()) / args.steps for x in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    loss = float(objs[:9].sum().item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, objs, fitter)

    if rank == 0:
        ms = 1000.0 * dt / args.steps
        per_view, per_frame = algorithmic_bytes(tables.V, tables.J, S, views)
        n_img = frames * views
        # batches above 16 384 images are rendered in several launches per iteration (engine.MAX_IMAGES_PER_LAUNCH): the roofline
        # figures are per launch, i.e. per slice of images
        launches_per_step = max(1, round(kern_n / max(args.steps, 1)))
        kern_avg_ms = kern_ms / max(kern_n, 1)
        img_per_launch = n_img / launches_per_step
        achieved = (img_per_launch * per_view) / (kern_avg_ms * 1e-3) / 1e9 if kern_n else 0.0
        iter_bytes = frames * (per_frame + views * per_view)
        # HBM bytes of one tile-kernel launch from the PMC passes committed under profiles/ (offline data of this round:
        # FETCH_SIZE and WRITE_SIZE need separate rocprofv3 passes, so they cannot be read inside this run); used only
        # when the recorded launch has the same number of images as this one.
        traffic = traffic_src = None
        sol = {}
        for tf in TRAFFIC_FILES:
            tpath = os.path.join(REPO, "profiles", tf)
            if not os.path.exists(tpath):
                continue
            tj = json.load(open(tpath)).get(args.workload)
            if tj and tj["images_per_launch"] == n_img:
                traffic = (tj["FETCH_SIZE_KB"] * tj["fetch_correction"] + tj["WRITE_SIZE_KB"]) * 1024.0
                traffic_src = f"offline PMC passes (FETCH_SIZE x{tj['fetch_correction']:g} + WRITE_SIZE per launch), profiles/{tf}"
                sq = tj.get("sq") or {}
                if sq.get("SQ_INSTS_VALU") and sq.get("SQ_BUSY_CYCLES"):
                    # speed-of-light model of DESIGN.md section 6 (same launch-size rule as `traffic`): the VALU pipes need 2 cycles per
                    # wave64 instruction on 1024 SIMD-32s; the record streams move `traffic` bytes at the achievable 6.29 TB/s
                    valu_floor = sq["SQ_INSTS_VALU"] * 2.0 / (N_SIMD * PEAK_CLOCK_HZ) * 1e3
                    stream_floor = traffic / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3
                    sol = {"valu_busy": sq["SQ_INSTS_VALU"] * 2.0 / (N_SIMD * sq["SQ_BUSY_CYCLES"] / 32.0),
                           "valu_insts_per_image": sq["SQ_INSTS_VALU"] / n_img, "valu_floor_ms": valu_floor, "stream_floor_ms": stream_floor,
                           "sol_ms": max(valu_floor, stream_floor),
                           "sol_note": "valu_busy = SQ_INSTS_VALU x 2 cycles / (1024 SIMDs x SQ_BUSY_CYCLES / 32 shader engines), from the "
                                       "committed SQ pass; sol_ms = max(VALU floor at 2.4 GHz, stream floor at 6.29 TB/s): what this algorithm "
                                       "(exact K = 100, every (face, pixel) record written once and read twice) could reach with both "
                                       "perfectly overlapped; DESIGN.md section 6"}
                break
        alg_launch = img_per_launch * per_view
        out = {
            # BASELINE.json's metric, verbatim.  One fit iteration = LBS + render + loss + backward + Adam over the frames a GPU holds
            # (weak scaling: every GPU holds `frames_per_gpu` frames and finishes its iteration at the same rate); `value` is the
            # whole-job aggregate the contract asks for: the per-GPU rate x the GPUs of the job
            "metric": "SMIL fit-iters/sec (LBS+render+loss) per GPU at 1/2/4/8 MI355X",
            "value": world * 1000.0 / ms,
            "unit": "fit-iters/s (sum over the job's GPUs; one fit-iter = one iteration over a GPU's %d frames x %d view(s))" % (frames, views),
            "value_per_gpu": 1000.0 / ms,
            "frame_iters_per_sec": world * frames / (dt / args.steps),
            "n_gpus": world,
            "rccl_ranks": (dist.get_world_size() if world > 1 else 1) if args.backend == "nccl" else 0,
            "rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "all": rank_ms},
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "rehearsal": bool(args.share_gpu or args.backend != "nccl"),
            "config": {"workload": wl["name"] + (f" [--frames {frames}]" if args.frames else ""), "frames_per_gpu": frames, "views": views, "image": S, "window": window,
                       "weights": synthetic.STAGE1_WEIGHTS, "w_temporal": synthetic.STAGE1_TEMPORAL, "faces_per_pixel": 100, "tie_rule": args.tie_rule,
                       "parallelism": f"frames sharded x{world}, all-reduce of shared-parameter gradients"},
            "final_loss": loss,
            "roofline": {"bound": "hbm", "kernel": "k_raster_dense<FUSED> (soft silhouette fwd + L1 + bwd)",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_over_algorithmic": (traffic / alg_launch) if traffic else None,
                         "traffic_achieved": (traffic / (kern_avg_ms * 1e-3) / 1e9) if (traffic and kern_n) else None,
                         "traffic_frac": (traffic / (kern_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (traffic and kern_n) else None,
                         **sol, "sol_frac": ((alg_launch / (sol["sol_ms"] * 1e-3) / 1e9) / HBM_PEAK_GBS) if sol else None,
                         "algorithmic_bytes_per_launch": alg_launch, "kernel_ms": kern_avg_ms, "launches_timed": kern_n,
                         "launches_per_step": launches_per_step, "images_per_launch": img_per_launch,
                         "algorithmic_bytes_per_image": per_view,
                         "iteration_frac": (iter_bytes / (ms * 1e-3) / 1e9) / HBM_PEAK_GBS,
                         "note": "achieved = algorithmic bytes (SURVEY.md 8(d): 36V + 20S^2 + 28J + 56 per image) / tile-kernel time from HIP "
                                 "events on its launch stream; traffic = HBM bytes the kernel really moved (its per-pair record streams), "
                                 "see DESIGN.md section 6"},
        }
        if parity is not None:
            out["parity_check"] = parity
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        if args.full and world == 1 and args.workload == "cfg2b" and not args.frames and not args.no_others:
            # the other BASELINE configurations as the driver sees them: five steps each, after the headline's timed region and
            # outside it (headline metric / config / dtype unchanged); the one-frame iteration is the only shape the unmodified
            # reference can run
            del fitter
            torch.cuda.empty_cache()
            # (a second or so of GPU time each: the whole GPU part of this run is then several seconds in one stretch)
            others = {k: time_other_workload(k, dev, steps={"cfg2": 200, "cfg3": 30, "cfg4": 60}[k]) for k in ("cfg2", "cfg3", "cfg4")}
            others["one_frame_eager"] = time_other_workload("cfg2", dev, steps=200, warmup=5, frames=1)
            others["one_frame_graph"] = time_other_workload("cfg2", dev, steps=200, warmup=5, frames=1, graph=True)
            # the headline workload with the reference's own choice among equal depths (SmilRasterSettings.tie_rule = 1): what the
            # faithful mode costs (kernel_ms / frac are the tile kernel's alone, the replay kernel runs behind it)
            others["cfg2b_tie_rule_reference_queue"] = time_other_workload(args.workload, dev, steps=40, frames=args.frames, tie_rule="reference_queue")
            # the reference's unchanged driver loop (the drop-in boundary) beside fit_step on the same configuration
            others["reference_loop_cfg2"] = time_reference_loop("cfg2", dev, epochs=100, fit_step_ms=others["cfg2"]["ms_per_step"])
            # the drop-in SMAL module on its own (the neural caller's shape): LBS forward + backward with a beta row per frame
            others["smal_call_stick_4096"] = time_smal_call("cfg2b", dev)
            others["smal_call_mouse_4096"] = time_smal_call("cfg3", dev)
            out["other_workloads"] = others
        print(json.dumps(out), flush=True)
        if parity is not None and not parity["ok"]:
            print(f"bench.py: parity check FAILED: {parity}", file=sys.stderr, flush=True)
            if world > 1:
                dist.destroy_process_group()
            raise SystemExit(3)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
