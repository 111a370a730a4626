"""Drop-in ``SMALFitter`` plus the fused whole-sequence fit step.

``SMALFitter`` keeps the reference's constructor, parameter names and ``forward(batch_range, weights,
stage_id) -> (loss, objs)`` / ``get_temporal`` / ``load_checkpoint`` contract
(reference smal_fitter/fitter.py:55-371).  Every arithmetic step - LBS, projection, soft silhouette, the six
loss terms and all their gradients - runs in HIP kernels of ``libsmilfit.so``; autograd only sees one node
per call whose backward hands out the gradients the kernels already produced.

``SMALFitter.fit_step`` is the fast path used by ``smilify_amd.optimize`` and ``bench.py``: one call = one
epoch of reference optimize_to_joints.py:147-175 over all frames of this rank (sum over windows of window
means + temporal terms, backward, Adam step), with no autograd graph and no per-window Python.

Extensions over the reference, needed for the batched / multi-view configurations:
``fov`` may have shape (1,), (views,) or (N*views,); ``log_beta_scales`` / ``betas_trans`` may be
(1,J,3) shared or (N,J,3) per frame; cameras may be given per view; targets are (N*views, ...).
"""
from __future__ import annotations

import math
import os
import pickle as pkl
import warnings
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import config as _config
from . import engine, fit_eval, fit_graph, model_io
from .cameras import FoVCameras
from .fit_epoch import INVALIDATED_BY, FitState, _FitWindow, _TemporalTerm, masks_part, targets_part, weights_part
from .p3d_renderer import Renderer
from .smal_torch import SMAL

OBJ_NAMES = ("joint", "limit", "pose", "splay", "betas", "sil_reproj")  # reference objs keys, in objs[] order
_WEIGHT_OF = {"joint": 0, "sil_reproj": 1, "betas": 2, "pose": 3, "limit": 4, "splay": 5}  # position of a term's weight (fitter.py:238)


def default_global_rotation() -> np.ndarray:
    """``eul_to_axis([-pi/2, 0, -pi/2])`` of reference fitter.py:206: nibabel's euler2angle_axis(z, y, x)
    composes R_x(x) R_y(y) R_z(z); at y = 0 the quaternion is (cx cz, sx cz, -sx sz, cx sz)."""
    hx = hz = -math.pi / 4
    q = np.array([math.cos(hx) * math.cos(hz), math.sin(hx) * math.cos(hz), -math.sin(hx) * math.sin(hz), math.cos(hx) * math.sin(hz)])
    angle = 2.0 * math.acos(q[0])
    return (q[1:] / np.linalg.norm(q[1:]) * angle).astype(np.float32)


def shape_prior_precision(shape_cov, n_betas: int) -> np.ndarray:
    """Cholesky factor of the regularised inverse shape covariance (reference fitter.py:170-175)."""
    cov = np.eye(n_betas) if shape_cov is None else np.asarray(shape_cov, np.float64)
    prec = np.linalg.cholesky(np.linalg.inv(cov + 1e-5 * np.eye(cov.shape[0])))
    return prec[:n_betas, :n_betas].astype(np.float32)


class _Prior:
    """Identity-precision pose prior (reference fitter.py:25-52); kept for API parity, evaluated in-kernel."""

    def __init__(self, n_joints: int, device):
        self.use_ind = np.ones(n_joints * 3, dtype=bool)
        self.use_ind[:3] = False
        self.use_ind_tch = torch.from_numpy(self.use_ind).float().to(device)


class SMALFitter(nn.Module):
    epoch_cache = True  # forward() may serve the windows of an epoch from one whole-batch evaluation (False: every call on its own)

    def __init__(self, device, data_batch, batch_size, shape_family=-1, use_unity_prior=False, rgb_only=False, *,
                 tables: Optional[model_io.SmilModelTables] = None, model_path: Optional[str] = None,
                 config: Optional[_config.FitterConfig] = None, views: int = 1, frame0: int = 0, n_frames_total: Optional[int] = None):
        super().__init__()
        self._cache = FitState()  # (first: the attribute hook below reaches for it)
        if use_unity_prior or shape_family != -1:
            raise NotImplementedError("the Unity / shape-family priors need MPI-licensed files that SMIL models do not use")
        self.device = engine.require_gpu(device)
        dev = self.device
        if tables is None:
            cfg0 = config or _config.current
            path = model_path or (cfg0.SMAL_FILE if cfg0 is not None else None)
            if path is None:
                raise ValueError("SMALFitter needs tables=, model_path= or config.SMAL_FILE")
            tables = model_io.load_model(path)
        self.config = config or _config.current or _config.FitterConfig.from_tables(tables, model_path)
        cfg = self.config
        self.rgb_only = rgb_only
        self.views = int(views)
        J, nB = tables.J, tables.nB
        if rgb_only:
            self.rgb_imgs = data_batch
            n_img = self.rgb_imgs.shape[0]
            self.sil_imgs = None
            self.target_joints = torch.zeros(n_img, len(cfg.CANONICAL_MODEL_JOINTS), 2)
            self.target_visibility = torch.zeros(n_img, len(cfg.CANONICAL_MODEL_JOINTS)).long()
        else:
            self.rgb_imgs, self.sil_imgs, self.target_joints, self.target_visibility = data_batch
            self.target_visibility = self.target_visibility.long()
        n_img = self.sil_imgs.shape[0] if self.sil_imgs is not None else self.rgb_imgs.shape[0]
        if n_img % self.views:
            raise ValueError(f"{n_img} target images is not a multiple of views={self.views}")
        self.num_images = n_img // self.views  # frames held by this rank
        self.image_size = int(self.sil_imgs.shape[-1] if self.sil_imgs is not None else self.rgb_imgs.shape[2])
        self.frame0 = int(frame0)
        self.n_frames_total = int(n_frames_total) if n_frames_total is not None else self.num_images
        self.use_unity_prior = False
        self.batch_size = batch_size
        self.n_betas = nB
        self.shape_family_list = np.array(shape_family)
        self.propagate_scaling = False
        N = self.num_images

        # shape prior learned from the scanned models, identity fallback (reference fitter.py:121-136,170-175)
        mean = tables.shape_mean_betas if (tables.shape_cov is not None and tables.shape_mean_betas is not None) else None
        self.mean_betas = (torch.zeros(nB) if mean is None else torch.from_numpy(np.asarray(mean, np.float32))[:nB]).to(dev).contiguous()
        self.betas_prec = torch.from_numpy(shape_prior_precision(tables.shape_cov if mean is not None else None, nB)).to(dev).contiguous()
        self.pose_prior = _Prior(J, dev)
        self.max_limits = torch.full((J - 1, 3), cfg.JOINT_LIMIT, device=dev)
        self.min_limits = -self.max_limits

        # parameters (names as in the reference: optimize_to_joints.py:118-144 addresses them by name)
        self.betas = nn.Parameter(self.mean_betas.clone())
        self.log_beta_scales = nn.Parameter(torch.zeros(N, J, 3, device=dev), requires_grad=False)
        self.betas_trans = nn.Parameter(torch.zeros(N, J, 3, device=dev), requires_grad=False)
        # global_rotation and joint_rotations are views of ONE (N,J,3) pose buffer so the kernels read them without
        # a concatenation; they stay ordinary leaf Parameters for torch.optim
        self._pose = torch.zeros(N, J, 3, device=dev)
        self._pose[:, 0] = torch.from_numpy(default_global_rotation()).to(dev)
        self.global_rotation = nn.Parameter(self._pose[:, 0])
        self.joint_rotations = nn.Parameter(self._pose[:, 1:])
        self.trans = nn.Parameter(torch.zeros(N, 3, device=dev))
        self.global_mask = torch.ones(1, 3, device=dev)
        self.rotation_mask = torch.ones(J - 1, 3, device=dev)

        self.smal_model = SMAL(dev, tables=tables, config=cfg)
        self.renderer = Renderer(self.image_size, dev, views=self.views, colour=bool(getattr(cfg, "RENDER_COLOUR", False)))
        self.renderer.bind_model(self.smal_model.device_model)
        self.renderer.mesh_color = torch.tensor(list(cfg.MESH_COLOR), dtype=torch.float32, device=dev)[None, None, :] / 255.0
        self.fov = nn.Parameter(self.renderer.cameras.fov.clone())  # (1,) = 60 deg

    # ---- plumbing --------------------------------------------------------------------------------------------
    @property
    def device_model(self) -> engine.DeviceModel:
        return self.smal_model.device_model

    # read-only views on the cached state (bench.py, tools and tests read these names)
    _epoch = property(lambda self: self._cache.epoch)
    _graph = property(lambda self: self._cache.graph)
    _sil_dev = property(lambda self: self._cache.sil)
    _sil_sum = property(lambda self: self._cache.sil_sum)
    _vis_dev = property(lambda self: self._cache.vis)

    def set_cameras(self, R, T, fov=None, aspect_ratio=None, principal_point=None):
        """Install per-view or per-image cameras; ``fov`` (if given) replaces the trainable parameter.  ``principal_point``: ``(k,2)``
        NDC offsets ``(px, py)`` of calibrated pinhole cameras or crop windows (``Renderer.set_camera_parameters``); a constant of the fit."""
        f = self.fov.data if fov is None else fov
        self.renderer.set_camera_parameters(R, T, f, aspect_ratio, principal_point)
        if fov is not None:
            self.fov = nn.Parameter(self.renderer.cameras.fov.clone())
        self._cache.invalidate("tables")  # a captured iteration holds the old camera tables' addresses

    def _refresh_targets(self, force: bool = True):
        """Upload the targets; ``force=False``: only if they were replaced, edited in place or declared stale."""
        c, dev = self._cache, self.device
        if not (force or c.targets_dirty or targets_part(self) != c.target_signature):
            return
        n_img = self.num_images * self.views
        if self.sil_imgs is not None:
            sil = self.sil_imgs.to(dev).reshape(n_img, self.image_size, self.image_size)
            if sil.dtype != torch.uint8:
                sil = sil.float()
                # binary masks (the usual case) are kept as bytes: a quarter of the memory and of the read traffic
                if bool(((sil == 0) | (sil == 1)).all()):
                    sil = sil.to(torch.uint8)
            c.sil = sil.contiguous()
            c.sil_sum = engine.image_abs_sum(c.sil)
        else:
            c.sil = c.sil_sum = None
        c.tj = self.target_joints.to(dev).float().contiguous()
        c.vis = self.target_visibility.to(dev).to(torch.int32).contiguous()
        canon = list(self.config.CANONICAL_MODEL_JOINTS)
        c.canon_identity = canon == list(range(self.smal_model.tables.J))
        c.canon = torch.tensor(canon, dtype=torch.int32, device=dev)
        c.targets_dirty = False
        c.target_signature = targets_part(self)

    def invalidate_targets(self):
        """Force a re-upload of the targets (in-place edits and re-assignments are detected automatically)."""
        self._cache.invalidate("targets")

    def invalidate_epoch(self):
        """Forget the cached epoch (after editing a parameter through ``.data`` or any other route autograd's version counters miss)."""
        self._cache.invalidate("parameters")

    def __setattr__(self, name, value):
        if name in INVALIDATED_BY:  # re-assigned targets / tables: what was cached read the old buffers
            self._cache.invalidate(INVALIDATED_BY[name])
        super().__setattr__(name, value)

    def _mask_table(self) -> torch.Tensor:
        """(J,3) = [global_mask ; rotation_mask] in ONE persistent device buffer, refreshed in place when a mask tensor was
        replaced or edited in place (the reference documents ``fitter.rotation_mask[25:32] = 0.0``): a captured iteration
        reads this buffer, so it sees the current masks at every replay."""
        key, cached = masks_part(self), self._cache.mask
        if cached is None or cached[0] != key:
            table = torch.cat([self.global_mask.reshape(1, 3), self.rotation_mask.reshape(-1, 3)], 0).float().contiguous()
            if cached is not None and cached[1].shape == table.shape and cached[1].device == table.device:
                cached[1].copy_(table)
                table = cached[1]
            cached = self._cache.mask = (key, table)
        return cached[1]

    def _pix_scale(self, fc, views: int, S: int) -> torch.Tensor:
        """Per-image weight of the silhouette term (w_reproj / (window size * views * S^2)): depends on the loss weights and
        the window layout only, so it is computed once per configuration, not once per iteration."""
        key, cached = (fc.N, views, S, fc.w_reproj, fc.window, fc.frame0, fc.N_total), self._cache.pix_scale
        if cached is None or cached[0] != key:
            cached = self._cache.pix_scale = (key, engine.pix_scale(fc, views, S, self.device))
        return cached[1]

    def _loss_and_grads(self, frames: Optional[Sequence[int]], weights, w_temp: float, window: Optional[int] = None,
                        halo_prev=None, halo_next=None, halo=None, window_terms: bool = False):
        """Evaluate every loss term and the gradient of their sum for ``frames`` (None = all frames of this rank): ``fit_eval``.

        Returns ``(objs (10,), grads)`` with full-size gradient tensors (zero rows outside ``frames``).
        ``window``: frames per loss window; None = the selected frames form one window (``forward`` semantics).
        ``halo``: an ``optimize.PendingHalo`` instead of ``halo_prev`` / ``halo_next`` - waited for right before the epilogue kernel,
        the only reader of the rows, so the messages travel while skinning and rasteriser run.  ``window_terms``: also return
        ``grads["_objs_win"]`` (windows, 6), the six terms of every window on its own (one more kernel: ``smil_window_terms``)."""
        self._refresh_targets(force=False)
        return fit_eval.Evaluation(self, frames, weights, w_temp, window).run(halo_prev, halo_next, halo, window_terms)

    # ---- reference API ---------------------------------------------------------------------------------------
    def print_grads(self, grad_output):
        """Debug hook of the reference (fitter.py:233-234): prints a gradient it is registered on."""
        print(grad_output)

    def forward(self, batch_range, weights, stage_id):
        """Reference fitter.py:236-335: ``(sum of the weighted terms, dict of the terms)`` for one window.  From the SECOND window
        requested under unchanged parameters on, all windows of the epoch are evaluated in one launch chain and this call - and
        every later one of the epoch - is served from it (``fit_epoch.FitState.serve``)."""
        wts = weights_part(weights)
        total, objs = self._cache.serve(self, batch_range, wts) or _FitWindow.apply(
            self, list(batch_range), list(wts), 0.0, self.betas, self.log_beta_scales, self.betas_trans, self._pose_leaf(), self.trans, self.fov)
        terms = objs.unbind(0)
        return total, {name: terms[k] for k, name in enumerate(OBJ_NAMES)
                       if wts[_WEIGHT_OF[name]] > 0 and not (name == "sil_reproj" and self.rgb_only)}

    def _pose_leaf(self):
        """Autograd handle tying the fused pose gradient to the two rotation Parameters."""
        return torch.cat([self.global_rotation[:, None], self.joint_rotations], dim=1)

    def get_temporal(self, w_temp):
        """Reference fitter.py:337-350: (joint_loss, global_loss, trans_loss) over consecutive frames - three scalars, each
        carrying its own graph like the reference's: the joint term depends on ``joint_rotations`` only, the global term on
        ``global_rotation`` only, the translation term on ``trans`` only, so the one evaluated gradient splits exactly."""
        joint, glob, tr = _TemporalTerm.apply(self, float(w_temp), self._pose_leaf(), self.trans)
        return joint, glob, tr

    def load_checkpoint(self, checkpoint_path, epoch):
        """Reference fitter.py:352-371: per-frame ``<frame>/<epoch>.pkl`` parameter dicts; betas/scales averaged."""
        beta_list, scale_list = [], []
        with torch.no_grad():
            for frame_id in range(self.num_images):
                with open(os.path.join(checkpoint_path, "{0:04}".format(frame_id), "{0}.pkl".format(epoch)), "rb") as f:
                    p = pkl.load(f)
                self.global_rotation[frame_id] = torch.from_numpy(np.asarray(p["global_rotation"])).float().to(self.device).reshape(3)
                self.joint_rotations[frame_id] = torch.from_numpy(np.asarray(p["joint_rotations"])).float().to(self.device).view(-1, 3)
                self.trans[frame_id] = torch.from_numpy(np.asarray(p["trans"])).float().to(self.device).reshape(3)
                beta_list.append(np.asarray(p["betas"]).reshape(-1)[: self.n_betas])
                scale_list.append(np.asarray(p["log_betascale"]))
        self.betas = nn.Parameter(torch.from_numpy(np.mean(beta_list, axis=0)).float().to(self.device))
        scales = torch.from_numpy(np.mean(scale_list, axis=0)).float().to(self.device).reshape(1, -1, 3)
        self.log_beta_scales = nn.Parameter(scales, requires_grad=self.log_beta_scales.requires_grad)

    def generate_visualization(self, image_exporter, apply_UE_transform=False, img_idx=0, mesh_scale=None, epoch=None):
        """Reference fitter.py:373-517, as far as this build goes: for every frame ``image_exporter.export(collage, batch_id,
        global_id, img_parameters, verts, faces, img_idx, epoch=epoch)`` with the SAME per-frame parameter dict (what the reference
        pickles as ``st{S}_ep{E}.pkl`` and ``load_checkpoint`` reads back), the same posed vertices (the ``.ply``) and a collage of the
        same layout (target | render | overlay | silhouette agreement | view from behind).  The reference's driver calls this
        every ``VIS_FREQUENCY`` epochs (optimize_to_joints.py:177-178), so the unchanged loop needs it to work.  With
        ``FitterConfig.RENDER_COLOUR`` the render, overlay and view-from-behind panels come from the HardPhong colour image
        (``Renderer.render_colour``, as the reference's render_texture=True); by default they show the soft silhouette in the mesh
        colour.  The joint markers (SMALJointDrawer, cv2) are visualisation code outside this build and are not drawn.
        Frames are posed and rendered by the HIP kernels; the collage is assembled on the host."""
        cfg, dev, views, S = self.config, self.device, self.views, self.image_size
        J = self.smal_model.tables.J
        faces_np = self.smal_model.faces.detach().cpu().numpy()
        color = torch.tensor([c / 255.0 for c in getattr(cfg, "MESH_COLOR", [0, 172, 223])], dtype=torch.float32).view(1, 3, 1, 1)
        rot = torch.tensor([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], device=dev)  # 180 degrees about y (fitter.py:388)
        cam_all = self.renderer.cameras
        W = int(self.batch_size) if self.batch_size else self.num_images
        try:
            with torch.no_grad():
                for j in range(0, self.num_images, W):
                    rows = list(range(j, min(self.num_images, j + W)))
                    idx = torch.tensor(rows, device=dev)
                    n = len(rows)
                    pick = lambda p_: (p_.detach() if p_.shape[0] == 1 else p_.detach().index_select(0, idx))  # noqa: E731
                    theta = torch.cat([(self.global_rotation.detach().index_select(0, idx) * self.global_mask)[:, None],
                                       self.joint_rotations.detach().index_select(0, idx) * self.rotation_mask], 1)
                    trans = self.trans.detach().index_select(0, idx)
                    verts, joints, _, _ = self.smal_model(self.betas.detach()[None].expand(n, -1), theta, betas_logscale=pick(self.log_beta_scales),
                                                          betas_trans=pick(self.betas_trans), propagate_scaling=self.propagate_scaling)
                    if apply_UE_transform:  # (the replicAnt convention: ten times larger about the root joint)
                        root = joints[:, :1]
                        verts, joints = (verts - root) * 10 + trans[:, None], (joints - root) * 10 + trans[:, None]
                    elif mesh_scale is not None:
                        sc = torch.as_tensor(mesh_scale, dtype=torch.float32, device=dev).reshape(-1, 1, 1)
                        root = joints[:, :1]
                        verts, joints = (verts - root) * sc + trans[:, None], (joints - root) * sc + trans[:, None]
                    else:
                        verts, joints = verts + trans[:, None], joints + trans[:, None]
                    canon = joints[:, list(cfg.CANONICAL_MODEL_JOINTS)].contiguous()
                    img_rows = (idx[:, None] * views + torch.arange(views, device=dev)[None]).reshape(-1)

                    def table(t_, per_row):  # camera tables with one row per image follow the window; shared / per-view ones stay
                        return t_ if t_ is None or t_.shape[0] != self.num_images * views else t_.index_select(0, img_rows)
                    fov = self.fov.detach().reshape(-1)
                    self.renderer.cameras = FoVCameras(table(cam_all.R, 9), table(cam_all.T, 3), table(fov, 1),
                                                       table(cam_all.aspect_ratio, 1), cam_all.znear, cam_all.zfar,
                                                       table(getattr(cam_all, "principal_point", None), 2))
                    faces_b = self.smal_model.faces[None].expand(n, -1, -1)
                    colour = self.renderer.colour
                    out = self.renderer(verts.contiguous(), canon, faces_b, render_texture=colour)
                    centre = verts.mean(1, keepdim=True)
                    out_rev = self.renderer(((verts - centre) @ rot.T).contiguous(), ((canon - centre) @ rot.T).contiguous(), faces_b,
                                            render_texture=colour)
                    first = torch.arange(n, device=dev) * views  # a frame's first view stands for it
                    sil = out[0].reshape(n * views, 1, S, S).index_select(0, first).cpu()
                    sil_rev = out_rev[0].reshape(n * views, 1, S, S).index_select(0, first).cpu()
                    take = (idx * views).cpu()
                    rgb = self.rgb_imgs[take].float().cpu()
                    target_sil = torch.zeros_like(sil) if (self.rgb_only or self.sil_imgs is None) else self.sil_imgs[take].float().cpu().reshape(n, 1, S, S)
                    if colour:  # the reference's panels (fitter.py:462-480): colour render, its overlay, colour view from behind
                        rendered = out[2].index_select(0, first).cpu()
                        rendered_rev = out_rev[2].index_select(0, first).cpu()
                    else:
                        rendered, rendered_rev = sil * color, sil_rev * color
                    agreement = (1.0 - (target_sil - sil).abs()).expand_as(rgb)
                    collage = torch.cat([rgb, rendered, 0.5 * rendered + 0.5 * rgb, agreement, rendered_rev], dim=3).clamp(0.0, 1.0)
                    for batch_id, global_id in enumerate(rows):
                        image_exporter.export((collage[batch_id].permute(1, 2, 0).numpy() * 255.0).astype(np.uint8), batch_id, global_id,
                                              self.export_parameters(global_id), verts, faces_np, img_idx, epoch=epoch)
        finally:
            self.renderer.cameras = cam_all

    def posed_mesh(self):
        """``(vertices (frames,V,3), canonical joints (frames,Jc,3))`` of the current parameters, in world space, without gradient:
        what a fit iteration renders."""
        with torch.no_grad():
            n = self.num_images
            theta = torch.cat([(self.global_rotation.detach() * self.global_mask)[:, None], self.joint_rotations.detach() * self.rotation_mask], 1)
            verts, joints, _, _ = self.smal_model(self.betas.detach()[None].expand(n, -1), theta, betas_logscale=self.log_beta_scales.detach(),
                                                  betas_trans=self.betas_trans.detach(), propagate_scaling=self.propagate_scaling)
            trans = self.trans.detach()[:, None]
            return (verts + trans).contiguous(), (joints + trans)[:, list(self.config.CANONICAL_MODEL_JOINTS)].contiguous()

    def joint_self_occlusion(self, tolerance: float, neighborhood: int = 1) -> torch.Tensor:
        """(frames * views, Jc) float32: 1 where the canonical joint of the current parameters is seen by the image's camera, 0 where
        the posed mesh itself hides it (``Renderer.keypoint_visibility`` through the fitter's own renderer and cameras, with the
        fitter's ``fov``).  ``tolerance`` (world units) must exceed the depth of the joints under the skin.  Reads only: target
        visibilities, the cached epoch and captured graphs stay as they are."""
        verts, canon = self.posed_mesh()
        cam_all = self.renderer.cameras
        try:
            self.renderer.cameras = FoVCameras(cam_all.R, cam_all.T, self.fov.detach().reshape(-1), cam_all.aspect_ratio, cam_all.znear, cam_all.zfar,
                                               getattr(cam_all, "principal_point", None))
            return self.renderer.keypoint_visibility(verts, canon, self.smal_model.faces[None].expand(verts.shape[0], -1, -1), tolerance, neighborhood)
        finally:
            self.renderer.cameras = cam_all

    def export_parameters(self, frame_id: int) -> Dict[str, np.ndarray]:
        """The per-frame dict the reference pickles (optimize_to_joints.py:48-63, fitter.py:241-261,507)."""
        ls = self.log_beta_scales.detach()
        bt = self.betas_trans.detach()
        return dict(
            global_rotation=(self.global_rotation.detach()[frame_id] * self.global_mask[0]).cpu().numpy(),
            joint_rotations=(self.joint_rotations.detach()[frame_id] * self.rotation_mask).cpu().numpy(),
            betas=self.betas.detach().cpu().numpy(), trans=self.trans.detach()[frame_id].cpu().numpy(),
            fov=self.fov.detach().reshape(-1)[min(frame_id, self.fov.numel() - 1)].cpu().numpy(),
            log_betascale=ls[min(frame_id, ls.shape[0] - 1)].cpu().numpy(), betas_trans=bt[min(frame_id, bt.shape[0] - 1)].cpu().numpy())

    # ---- fused epoch (fast path) -----------------------------------------------------------------------------
    def begin_stage(self, lr: float, fov_lr: float = 1.0, betas=(0.5, 0.999), eps: float = 1e-8):
        """New Adam state per stage, like the reference's new optimiser per stage (optimize_to_joints.py:117-127)."""
        self._cache.invalidate("stage")
        self._cache.adam_hyper = dict(lr=float(lr), fov_lr=float(fov_lr), betas=betas, eps=eps)

    def _adam_items(self, grads: Dict[str, Optional[torch.Tensor]], first_step: Optional[int]):
        """``(param, grad, state, lr)`` of every parameter that received a gradient; the moments of a parameter seen for the first time
        are created, its own step count starting at the optimiser's step ``first_step`` (None: nothing is created, KeyError instead)."""
        c, h = self._cache, self._cache.adam_hyper
        for name, g in grads.items():
            if g is None:
                continue
            p = self._pose if name == "pose" else getattr(self, name).data
            st = c.adam.get(name) if first_step is not None else c.adam[name]
            if st is None:
                st = c.adam[name] = dict(m=torch.zeros_like(p), v=torch.zeros_like(p), t0=first_step - 1)
            yield p, g, st, h["fov_lr"] if name == "fov" else h["lr"]

    def apply_adam(self, grads: Dict[str, Optional[torch.Tensor]], advance: bool = True):
        """torch.optim.Adam(betas=(0.5,0.999)) semantics on every parameter that received a gradient.  ``advance=False``:
        a second group of the same optimiser step (the shared parameters, once their all-reduced gradient has arrived)."""
        c, h = self._cache, self._cache.adam_hyper
        if advance:
            c.adam_step += 1
        items = [(p, g.contiguous(), st["m"], st["v"], lr, c.adam_step - st["t0"]) for p, g, st, lr in self._adam_items(grads, c.adam_step)]
        if items:  # one launch for all of them
            engine.adam_step_multi(items, h["betas"][0], h["betas"][1], h["eps"])
            c.invalidate("parameters")  # (written through .data: the parameters' version counters do not move)

    def fit_step(self, weights, w_temp: float, window: Optional[int] = None, halo_prev=None, halo_next=None,
                 shared_grad_hook=None, halo=None):
        """One epoch over all frames of this rank: losses + gradients + Adam.  Returns objs (10,) (device).

        Several ranks: ``shared_grad_hook(block)`` receives the shared block - one contiguous tensor ``[10 loss terms | d_betas
        | d_fov | shared scale-table gradients]`` - right after backward, sums it over the ranks IN PLACE and returns a handle
        (``optimize.allreduce_block``).  The per-frame parameters take their Adam step while that collective is in flight;
        the shared ones after ``handle.wait()``."""
        window = self.config.WINDOW_SIZE if window is None else window
        objs, grads = self._loss_and_grads(None, weights, w_temp, window=window, halo_prev=halo_prev, halo_next=halo_next, halo=halo)
        if shared_grad_hook is None:
            self.apply_adam(grads)
            return objs
        block = self._cache.block  # (its layout says which gradients live in the tensor the ranks sum)
        handle = shared_grad_hook(block.tensor)
        base = block.tensor.untyped_storage().data_ptr()
        stray = [k for k in block.shared if grads[k] is not None and grads[k].untyped_storage().data_ptr() != base]
        assert not stray, f"shared gradients outside the shared block: {stray}"  # (the ranks would leave them un-reduced)
        self.apply_adam({k: g for k, g in grads.items() if k not in block.shared})
        if handle is not None:
            handle.wait()
        self.apply_adam({k: g for k, g in grads.items() if k in block.shared}, advance=False)
        return objs

    def fit_step_graph(self, weights, w_temp: float, window: Optional[int] = None):
        """``fit_step`` for a single rank, captured once per (stage, weights) in a hipGraph and replayed afterwards (``fit_graph``)."""
        return fit_graph.step(self, weights, w_temp, window)

    def fit_step_graph_ranks(self, weights, w_temp: float, window: Optional[int], rank: int, world: int, group, shared_grad_hook,
                             host_staged: bool = False):
        """``fit_step`` of one rank among several as TWO hipGraphs with the collective between them (``fit_graph``)."""
        return fit_graph.step(self, weights, w_temp, window, (rank, world), group, shared_grad_hook, host_staged)

    def straddling_faces(self) -> int:
        """Faces of the most recent silhouette launch with one or two vertices nearer than ``z_clip = znear / 2``.  They are cut
        at the plane like pytorch3d's ``clip_faces`` does (left on by the reference's settings, p3d_renderer.py:36-47): the
        part in front is rendered.  A non-zero count still deserves a look - the mesh has reached the camera - so the first
        one warns; faces beyond the per-image clip tables (1024 cut faces per image) are rendered unclipped and always
        reported.  Synchronises the stream (call it between stages, not per iteration)."""
        if self.device_model._ws is None:
            return 0
        st = engine.raster_stats(self.device_model, self.num_images * self.views)
        n, lost = int(st["straddling_faces"]), int(st["unclipped_faces"])
        cd = self._cache.clip_depth  # (the buffer of the LAST evaluation only: other sizes' counters are stale)
        dropped = int(cd.counter.tolist()[1]) if cd is not None else 0  # (both counters in one copy)
        if dropped:  # (more cut edges in one call than ClipDepth.capacity entries: their depth gradients were left out, never silently)
            warnings.warn(f"{dropped} depth-gradient entries of cut edges did not fit engine.ClipDepth (capacity {cd.capacity}) in the "
                          "last evaluation and were dropped.", RuntimeWarning, stacklevel=2)
        if n and not self._cache.warned_straddling:
            self._cache.warned_straddling = True
            warnings.warn(f"{n} mesh faces straddle the camera's clipping plane (z_clip = znear / 2) and were cut there, as the "
                          f"reference's rasteriser does ({lost} of them beyond the clip tables: rendered unclipped). The mesh has "
                          "probably drifted into the camera (check `trans`).", RuntimeWarning, stacklevel=2)
        return n

    def boundary_rows(self):
        """(first, last) parameter rows [pose, trans] of this shard for the temporal halo exchange: two rows are sliced, the
        parameter matrix is not touched."""
        pose, trans = self._pose.detach(), self.trans.detach()
        row = lambda i: torch.cat([pose[i].reshape(-1), trans[i].reshape(-1)])  # noqa: E731
        return row(0), row(self.num_images - 1)
