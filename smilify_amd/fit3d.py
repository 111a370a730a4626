"""Drop-ins for the reference's 3-D registration program (fitter_3d/trainer.py, fitter_3d/optimise.py) on the HIP path.

``fitter_3d/trainer.py`` runs unchanged once its pytorch3d imports read::

    from smilify_amd.fit3d import sample_points_from_meshes, chamfer_distance, mesh_edge_loss, \\
        mesh_laplacian_smoothing, mesh_normal_consistency
    from smilify_amd.mesh3d import Meshes

and this module carries its ``SMAL3DFitter`` / ``SMALParamGroup`` / ``Stage`` / ``StageManager`` as well, with the SMAL half on the
existing LBS kernels and every loss on the kernels of ``csrc/mesh3d.hip``.  Each loss is a ``torch.autograd.Function`` whose forward
computes the loss and its gradient in one launch sequence; backward scales that gradient.

Deviations: sampling draws from a Philox counter-based generator keyed by a 64-bit seed taken from torch's
default CPU generator, so ``torch.manual_seed`` makes runs reproducible but the points differ from pytorch3d's (torch.multinomial /
torch.rand streams).  Out of scope and raising: the SDF term, loss / mesh plots, normals / lengths / norm=1 in chamfer_distance,
the cot / cotcurv Laplacians.

Run as ``python -m smilify_amd.fit3d --model MODEL.npz --mesh_dir DIR [--yaml_src CFG.yaml]`` (fitter_3d/optimise.py).
"""
from __future__ import annotations

import argparse
import os
from math import ceil
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, engine
from . import config as _config
from .fitter import shape_prior_precision
from .mesh3d import Meshes, load_meshes
from .smal_torch import SMAL

default_weights = dict(w_chamfer=1.0, w_edge=1.0, w_normal=0.01, w_laplacian=0.1, w_sdf=0.5)  # trainer.py:25-27
SPLIT_TARGET_MESHES_INTO_BATCHES_OF_SIZE = 0  # reference config.py:24 (<= 0: all target meshes in one batch)


# ---- losses ---------------------------------------------------------------------------------------------------------------------
def _gpu_f32(t: torch.Tensor) -> torch.Tensor:
    engine.require_gpu(t.device)
    return t.detach().to(torch.float32).contiguous()


def sample_points_from_meshes(meshes: Meshes, num_samples: int = 10000, return_normals: bool = False, return_textures: bool = False):
    """(N, num_samples, 3) points on the surfaces of ``meshes``, faces chosen with probability proportional to their area
    (pytorch3d.ops.sample_points_from_meshes, trainer.py:376).  No gradient: raises if the vertices require one."""
    if return_normals or return_textures:
        raise NotImplementedError("sample_points_from_meshes: return_normals / return_textures are not supported")
    vl = meshes.verts_list()
    if any(v.requires_grad for v in vl):
        raise NotImplementedError("sample_points_from_meshes: the HIP sampler has no gradient; detach the vertices first")
    pts, _ = sample_points_with_faces(meshes, num_samples)
    return pts


def sample_points_with_faces(meshes: Meshes, num_samples: int, seed: Optional[int] = None):
    """(points (N,S,3), face index within its mesh (N,S) int32).  ``seed`` None: a 63-bit value from torch's default generator."""
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
    faces, face_off, cum = meshes.sampling_tables()
    verts = _gpu_f32(meshes.verts_packed())
    return engine.sample_points(verts, faces, face_off, cum, len(meshes), int(num_samples), seed, want_faces=True)


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, single_directional, point_sum, batch_sum):
        want = x.requires_grad or y.requires_grad
        loss, _, _, dx, dy = engine.chamfer(_gpu_f32(x), _gpu_f32(y), single_directional, point_sum, batch_sum, want_grad=want)
        ctx.save_for_backward(dx, dy) if want else ctx.save_for_backward()
        ctx.want = want
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.want:
            return None, None, None, None, None
        dx, dy = ctx.saved_tensors
        return dx * g, dy * g, None, None, None


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None, batch_reduction="mean",
                     point_reduction="mean", norm: int = 2, single_directional: bool = False, abs_cosine: bool = True):
    """pytorch3d.loss.chamfer_distance for (N,P1,3) / (N,P2,3) tensors without lengths or normals: returns (loss, None)."""
    if x_lengths is not None or y_lengths is not None or x_normals is not None or y_normals is not None or weights is not None:
        raise NotImplementedError("chamfer_distance: lengths, normals and weights are not supported")
    if norm != 2:
        raise NotImplementedError("chamfer_distance: only norm=2")
    if point_reduction not in ("mean", "sum") or batch_reduction not in ("mean", "sum"):
        raise NotImplementedError("chamfer_distance: point_reduction / batch_reduction must be 'mean' or 'sum'")
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dim() == 3 and y.dim() == 3 and x.shape[2] == 3
            and y.shape[2] == 3 and x.shape[0] == y.shape[0]):
        raise ValueError("chamfer_distance: x (N,P1,3) and y (N,P2,3) tensors")
    loss = _ChamferFn.apply(x, y, bool(single_directional), point_reduction == "sum", batch_reduction == "sum")
    return loss, None


class _RegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, topo, terms):
        out, de, dn, dl = engine.mesh_regularisers(topo, _gpu_f32(verts), terms, want_grad=verts.requires_grad)
        ctx.grads = (de, dn, dl)
        return out

    @staticmethod
    def backward(ctx, g):
        d = None
        for k, gk in enumerate(ctx.grads):
            if gk is not None:
                d = gk * g[k] if d is None else d + gk * g[k]
        ctx.grads = None
        return d, None, None


def mesh_regularisers(meshes: Meshes, edge=True, normal=True, laplacian=True) -> torch.Tensor:
    """(3,) = mesh_edge_loss, mesh_normal_consistency, mesh_laplacian_smoothing("uniform") of meshes that share one face array, in
    one kernel (terms not asked for are 0)."""
    terms = (_lib.REG_EDGE if edge else 0) | (_lib.REG_NORMAL if normal else 0) | (_lib.REG_LAPLACIAN if laplacian else 0)
    topo = meshes.topology()
    verts = meshes.verts_padded()
    return _RegFn.apply(verts, topo.device(verts.device), terms)


def mesh_edge_loss(meshes: Meshes, target_length: float = 0.0):
    if target_length != 0.0:
        raise NotImplementedError("mesh_edge_loss: only target_length=0 (fitter_3d's use)")
    return mesh_regularisers(meshes, True, False, False)[0]


def mesh_normal_consistency(meshes: Meshes):
    return mesh_regularisers(meshes, False, True, False)[1]


def mesh_laplacian_smoothing(meshes: Meshes, method: str = "uniform"):
    if method != "uniform":
        raise NotImplementedError(f"mesh_laplacian_smoothing: method '{method}' (only 'uniform')")
    return mesh_regularisers(meshes, False, False, True)[2]


# ---- model ----------------------------------------------------------------------------------------------------------------------
def get_meshes(verts, faces, device="cuda"):
    return Meshes(verts=verts, faces=faces).to(device)


class SMAL3DFitter(nn.Module):
    """trainer.py:39-246: per-mesh SMAL parameters (betas, log_beta_scales, betas_trans, global_rot, trans, joint_rot,
    deform_verts) posed by the HIP ``SMAL``.  The model comes from ``model_path`` / ``tables`` / ``config.current.SMAL_FILE``."""

    def __init__(self, batch_size=1, device="cuda", shape_family=-1, model_path=None, tables=None):
        super().__init__()
        self.device = device
        self.batch_size = batch_size
        self.smal_model = SMAL(device, shape_family_id=shape_family, model_path=model_path, tables=tables)
        t = self.smal_model.tables
        self.n_betas = t.nB
        has_prior = t.shape_cov is not None and t.shape_mean_betas is not None
        mean = np.asarray(t.shape_mean_betas, np.float32)[: t.nB] if has_prior else np.zeros(t.nB, np.float32)
        self.mean_betas = torch.from_numpy(mean).to(device)
        self.betas_prec = torch.from_numpy(shape_prior_precision(t.shape_cov if has_prior else None, t.nB)).to(device)
        self.betas = nn.Parameter(self.mean_betas.unsqueeze(0).repeat(batch_size, 1))
        self.kintree_table = torch.stack([torch.from_numpy(t.parents.astype(np.int64)), torch.arange(t.J)]).to(device)
        self.n_joints = t.J
        self.log_beta_scales = nn.Parameter(torch.zeros(batch_size, self.n_joints, 3, device=device))
        self.betas_trans = nn.Parameter(torch.zeros(batch_size, self.n_joints, 3, device=device))
        self.global_rot = nn.Parameter(torch.zeros(batch_size, 3, device=device))  # eul_to_axis([0, 0, 0])
        self.trans = nn.Parameter(torch.zeros(batch_size, 3, device=device))
        self.joint_rot = nn.Parameter(torch.zeros(batch_size, t.J - 1, 3, device=device))
        self.global_mask = torch.ones(1, 3, device=device)
        self.rotation_mask = torch.ones(t.J - 1, 3, device=device)
        self.faces = self.smal_model.faces.unsqueeze(0).repeat(batch_size, 1, 1)
        self.deform_verts = nn.Parameter(torch.zeros(batch_size, t.V, 3, device=device))

    def get_joint_scales(self, log_beta_scales_arg=None):
        s = torch.exp(log_beta_scales_arg if log_beta_scales_arg is not None else self.log_beta_scales)
        for j in range(self.n_joints):
            p = int(self.kintree_table[0, j])
            if p != j and 0 <= p < s.shape[1]:
                s[:, j] = s[:, j] * s[:, p]
        return s

    def forward(self, betas=None, global_rot=None, joint_rot=None, trans=None, log_beta_scales=None, betas_trans=None,
                deform_verts=None, return_joints=False):
        pick = lambda a, b: a if a is not None else b  # noqa: E731
        theta = torch.cat([pick(global_rot, self.global_rot).unsqueeze(1), pick(joint_rot, self.joint_rot)], dim=1)
        verts, joints, _, _ = self.smal_model(pick(betas, self.betas), theta, trans=pick(trans, self.trans),
                                              betas_logscale=pick(log_beta_scales, self.log_beta_scales),
                                              betas_trans=pick(betas_trans, self.betas_trans))
        verts = verts + pick(deform_verts, self.deform_verts)
        return (verts, joints) if return_joints else verts


class SMALParamGroup:
    """trainer.py:249-291: the parameters each scheme optimises, with optional per-parameter learning rates."""

    param_map = {
        "init": ["global_rot", "trans"],
        "init_rot_lock": ["trans", "log_beta_scales"],
        "init_rot_lock_trans": ["trans", "betas_trans"],
        "init_rot_lock_trans_scale": ["trans", "betas_trans", "log_beta_scales"],
        "default": ["global_rot", "joint_rot", "trans", "betas", "log_beta_scales"],
        "default_with_betas_trans": ["global_rot", "joint_rot", "trans", "betas", "log_beta_scales", "betas_trans"],
        "shape": ["global_rot", "trans", "betas", "log_beta_scales", "betas_trans"],
        "pose": ["global_rot", "trans", "joint_rot", "betas", "log_beta_scales", "betas_trans"],
        "deform": ["deform_verts"],
        "all": ["global_rot", "trans", "joint_rot", "betas", "log_beta_scales", "betas_trans", "deform_verts"],
    }

    def __init__(self, model, group="smbld", lrs=None):
        self.model = model
        self.group = group
        assert group in self.param_map, f"Group {group} not in list of available params: {list(self.param_map.keys())}"
        self.lrs = dict(lrs) if lrs is not None else {}

    def __iter__(self):
        out = []
        for name in self.param_map[self.group]:
            d = {"params": [getattr(self.model, name)]}
            if name in self.lrs:
                d["lr"] = self.lrs[name]
            out.append(d)
        return iter(out)


class Stage:
    """trainer.py:294-509: one optimisation stage (Adam over a scheme's parameters, chamfer to 3000 fresh target samples per
    iteration plus the mesh regularisers)."""

    def __init__(self, nits: int, scheme: str, smal_3d_fitter: SMAL3DFitter, target_meshes: Meshes, mesh_names=(), name="optimise",
                 loss_weights=None, lr=1e-3, out_dir="static_fits_output", custom_lrs=None, device="cuda", plot_normals=False,
                 sample_size=1000, sdf_values=None, source_sdf_values=None, visualize_sdf_loss=False, sdf_vis_frequency=10):
        self.n_it = nits
        self.name = name
        self.out_dir = out_dir
        self.target_meshes = target_meshes
        self.mesh_names = list(mesh_names)
        self.smal_3d_fitter = smal_3d_fitter
        self.device = device
        self.plot_normals = plot_normals
        self.loss_weights = default_weights.copy()
        if loss_weights is not None:
            self.loss_weights.update(loss_weights)
        self.sample_size = sample_size
        if (sdf_values is not None or source_sdf_values is not None) and self.loss_weights["w_sdf"] > 0:
            raise NotImplementedError("the SDF term (w_sdf with sdf_values) is not supported on the HIP path")
        if visualize_sdf_loss:
            raise NotImplementedError("SDF loss visualisation is not supported")
        self.sdf_values = self.source_sdf_values = None
        self.losses_to_plot = []
        if custom_lrs is not None:
            for attr in custom_lrs:
                assert hasattr(smal_3d_fitter, attr), f"attr '{attr}' not in SMAL."
        self.param_group = SMALParamGroup(smal_3d_fitter, scheme, custom_lrs)
        self.scheduler = None
        self.optimizer = torch.optim.Adam(self.param_group, lr=lr)
        self.src_verts = smal_3d_fitter().detach()
        self.faces = smal_3d_fitter.faces.detach()
        self.src_mesh = get_meshes(self.src_verts, self.faces, device=device)
        self.n_verts = self.src_verts.shape[1]
        self.last_target_samples = None
        self.consider_loss = lambda loss_name: self.loss_weights[f"w_{loss_name}"] > 0

    def forward(self, src_mesh: Meshes, iteration=0):
        loss = 0
        comps = {}
        target_verts = sample_points_from_meshes(self.target_meshes, 3000)
        self.last_target_samples = target_verts
        if self.consider_loss("chamfer"):
            comps["chamfer"], _ = chamfer_distance(target_verts, src_mesh.verts_padded())
            loss = loss + self.loss_weights["w_chamfer"] * comps["chamfer"]
        use = [self.consider_loss(k) for k in ("edge", "normal", "laplacian")]
        if any(use):  # the three regularisers in one kernel
            reg = mesh_regularisers(src_mesh, *use)
            for k, on, r in zip(("edge", "normal", "laplacian"), use, reg.unbind(0)):
                if on:
                    comps[k] = r
                    loss = loss + self.loss_weights[f"w_{k}"] * r
        return loss, comps

    def step(self, epoch):
        new_src_verts = self.smal_3d_fitter()
        offsets = new_src_verts - self.src_verts
        new_src_mesh = self.src_mesh.offset_verts(offsets.view(-1, 3))
        loss, comps = self.forward(new_src_mesh, iteration=epoch)
        loss.backward()
        self.optimizer.step()
        return loss, comps

    def plot(self):
        raise NotImplementedError("mesh plots are not part of the HIP path (loss histories stay on the Stage)")

    def run(self, plot=False):
        if plot:
            raise NotImplementedError("mesh plots are not part of the HIP path (loss histories stay on the Stage)")
        comps = {}
        for i in range(self.n_it):
            self.optimizer.zero_grad()
            loss, comps = self.step(i)
            self.losses_to_plot.append(loss.detach())
            if not hasattr(self, "loss_components_to_plot"):
                self.loss_components_to_plot = {k: [] for k in comps}
            for k, v in comps.items():
                self.loss_components_to_plot[k].append(v.detach())
        if comps:
            print(f"\nFinal loss components for stage {self.name}:")
            for k, v in comps.items():
                print(f"{k}: {v.item():.6f}")

    def save_npz(self, labels=None):
        out = {}
        for p in ["global_rot", "joint_rot", "betas", "log_beta_scales", "trans", "deform_verts", "betas_trans"]:
            out[p] = getattr(self.smal_3d_fitter, p).cpu().detach().numpy()
        with torch.no_grad():
            out["verts"] = self.smal_3d_fitter().cpu().numpy()
        out["faces"] = self.faces.cpu().detach().numpy()
        out["labels"] = labels
        np.savez(os.path.join(self.out_dir, f"{self.name}.npz"), **out)


class StageManager:
    """trainer.py:511-582 without the plots."""

    def __init__(self, out_dir="static_fits_output", labels=None, plot_normals=False):
        self.stages = []
        self.out_dir = out_dir
        self.labels = labels
        self.plot_normals = plot_normals

    def add_stage(self, stage):
        self.stages.append(stage)

    def run(self):
        for stage in self.stages:
            stage.run(plot=False)
            stage.save_npz(labels=self.labels)


# ---- optimise.py ----------------------------------------------------------------------------------------------------------------
def combine_stage_results(results_dir, stage_names, n_batches):
    """optimise.py:65-95: one .npz per stage from the per-batch files (faces kept once), the batch files removed."""
    for stage_name in stage_names:
        combined = None
        for b in range(n_batches):
            path = os.path.join(results_dir, f"{stage_name}_batch_{b}.npz")
            if not os.path.exists(path):
                continue
            d = dict(np.load(path, allow_pickle=True))
            if combined is None:
                combined = d
            else:
                for k in combined:
                    if k != "faces":
                        combined[k] = np.concatenate([combined[k], d[k]], axis=0)
        if combined is not None:
            np.savez(os.path.join(results_dir, f"{stage_name}.npz"), **combined)
            for b in range(n_batches):
                path = os.path.join(results_dir, f"{stage_name}_batch_{b}.npz")
                if os.path.exists(path):
                    os.remove(path)


def get_mesh_files(mesh_dir, frame_step=1):
    return sorted(os.path.join(mesh_dir, f) for f in os.listdir(mesh_dir) if f.endswith(".obj"))[::frame_step]


def build_parser():
    p = argparse.ArgumentParser(description="Register the SMIL model to 3-D scans (fitter_3d/optimise.py on the HIP path)")
    p.add_argument("--model", type=str, default=None, help="SMIL model (.pkl / .npz); default: smilify_amd.config.current.SMAL_FILE")
    p.add_argument("--results_dir", type=str, default="fit3d_results")
    p.add_argument("--mesh_dir", type=str, required=True)
    p.add_argument("--frame_step", type=int, default=1)
    p.add_argument("--shape_family_id", type=int, default=-1)
    p.add_argument("--yaml_src", type=str, default=None)
    p.add_argument("--scheme", type=str, default="default", choices=list(SMALParamGroup.param_map.keys()))
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--nits", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=None,
                   help="SPLIT_TARGET_MESHES_INTO_BATCHES_OF_SIZE (reference config.py:24); <= 0: one batch")
    p.add_argument("--device", type=str, default="cuda")
    return p


def main(args):
    stage_options = None
    if args.yaml_src is not None:
        import yaml

        with open(args.yaml_src) as fh:
            cfg = yaml.load(fh, Loader=yaml.FullLoader)
        stage_options = cfg["stages"]
        for k, v in (cfg.get("args") or {}).items():
            setattr(args, k, v)
    if args.model is None and (_config.current is None or _config.current.SMAL_FILE is None):
        raise ValueError("--model is required when smilify_amd.config.current names no SMAL_FILE")
    mesh_files = get_mesh_files(args.mesh_dir, args.frame_step)
    if not mesh_files:
        raise FileNotFoundError(f"no .obj files in {args.mesh_dir}")
    n_total = len(mesh_files)
    bs = args.batch_size if args.batch_size is not None else SPLIT_TARGET_MESHES_INTO_BATCHES_OF_SIZE
    if bs <= 0:
        bs = n_total
    n_batches = ceil(n_total / bs)
    stage_names = []
    os.makedirs(args.results_dir, exist_ok=True)
    for b in range(n_batches):
        files = mesh_files[b * bs:(b + 1) * bs]
        names = [os.path.basename(f) for f in files]
        _, targets = load_meshes(mesh_files=files, device=args.device)
        manager = StageManager(out_dir=args.results_dir, labels=names)
        model = SMAL3DFitter(batch_size=len(targets), device=args.device, shape_family=args.shape_family_id, model_path=args.model)
        kw = dict(target_meshes=targets, smal_3d_fitter=model, out_dir=args.results_dir, device=args.device, mesh_names=names)
        if stage_options is not None:
            for stage_name, skw in stage_options.items():
                manager.add_stage(Stage(name=f"{stage_name}_batch_{b}" if n_batches > 1 else stage_name, **skw, **kw))
                if b == 0:
                    stage_names.append(stage_name)
        else:
            manager.add_stage(Stage(scheme=args.scheme, nits=args.nits, lr=args.lr, name=f"stage_batch_{b}" if n_batches > 1 else "stage", **kw))
            if b == 0:
                stage_names.append("stage")
        manager.run()
    if n_batches > 1:
        combine_stage_results(args.results_dir, stage_names, n_batches)
    return stage_names


if __name__ == "__main__":
    main(build_parser().parse_args())
