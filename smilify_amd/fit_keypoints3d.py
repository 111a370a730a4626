"""Sequence fitter for 3-D keypoint tracks: the model's posed joints against triangulated keypoints, no mesh and no renderer.

``KeypointFitter3D`` holds the parameters of ``SMALFitter`` under the same names and fits them to ``target_keypoints (N,Jc,3)``.  An
iteration is three launches: ``smil_kp3d_fit_eval`` (chain, joints, the 3-D term and its backward of every frame in one kernel,
csrc/joints.hip), ``smil_prior_losses(accumulate=1)`` (mask, train flags, priors, temporal terms) and ``smil_adam_step_multi_bc64``
(the Adam step of ``smil_adam_step_multi`` with the bias corrections formed in double, as ``torch.optim.Adam`` forms them).  Nothing
synchronises the host.  The term (objs[9]; windows as in ``SMALFitter``):

    w_k3d sum_w 1/(3 Jc b_w) sum_{n in w} sum_c vis[n,c] wj[c] rho(|joints[n, canon[c]] - target[n,c]|^2)

``rho(s) = s``, or the soft-L1 ``2 sigma^2 (sqrt(1 + s / sigma^2) - 1)`` with ``robust_scale = sigma > 0``.  A target row that is exactly
(0,0,0) or holds a non-finite entry is invisible.

Not supported: models with pose blend shapes (``joints.JointTables`` raises), per-frame scale tables (``log_beta_scales`` and
``betas_trans`` are one shared (J,3) table each), several ranks and hipGraph capture of the step.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, align as _align
from . import config as _config
from . import engine, model_io
from .fitter import default_global_rotation, shape_prior_precision
from .joints import JointTables


class KeypointFitter3D(nn.Module):
    def __init__(self, device, target_keypoints, visibility=None, *, tables: Optional[model_io.SmilModelTables] = None,
                 model_path: Optional[str] = None, config: Optional[_config.FitterConfig] = None, canonical_joints=None,
                 joint_weights=None, robust_scale: float = 0.0):
        super().__init__()
        self.device = dev = engine.require_gpu(device)
        if tables is None:
            cfg0 = config or _config.current
            path = model_path or (cfg0.SMAL_FILE if cfg0 is not None else None)
            if path is None:
                raise ValueError("KeypointFitter3D needs tables=, model_path= or config.SMAL_FILE")
            tables = model_io.load_model(path)
        self.tables = tables
        self.config = cfg = config or _config.current or _config.FitterConfig.from_tables(tables, model_path)
        self.joint_tables = engine.DeviceJointTables(JointTables.from_tables(tables), dev)
        J, nB = tables.J, tables.nB
        target = torch.as_tensor(target_keypoints)
        if target.dim() != 3 or target.shape[-1] != 3:
            raise ValueError(f"target_keypoints must be (N,Jc,3), got {tuple(target.shape)}")
        N, Jc = int(target.shape[0]), int(target.shape[1])
        canon = list(cfg.CANONICAL_MODEL_JOINTS if canonical_joints is None else canonical_joints)
        if len(canon) != Jc or any(not 0 <= int(c) < J for c in canon):
            raise ValueError(f"canonical_joints must name {Jc} joints of 0..{J - 1}, got {canon}")
        self.num_images, self.n_betas = N, nB
        self.propagate_scaling = False
        self.robust_scale = float(robust_scale)
        if not np.isfinite(self.robust_scale) or self.robust_scale < 0:
            raise ValueError(f"robust_scale must be finite and not negative, got {robust_scale}")
        self.canonical_joints = torch.tensor(canon, dtype=torch.int32, device=dev)
        self.target_keypoints = target.to(device=dev, dtype=torch.float32).contiguous()
        self.target_visibility = None
        if visibility is not None:
            vis = torch.as_tensor(visibility)
            if tuple(vis.shape) != (N, Jc):
                raise ValueError(f"visibility must be ({N},{Jc}), got {tuple(vis.shape)}")
            self.target_visibility = (vis != 0).to(device=dev, dtype=torch.uint8).contiguous()
        self.joint_weights = None
        if joint_weights is not None:
            wj = torch.as_tensor(joint_weights, dtype=torch.float64)
            if tuple(wj.shape) != (Jc,) or not bool(torch.isfinite(wj).all()) or bool((wj < 0).any()):
                raise ValueError(f"joint_weights must be ({Jc},), finite and not negative")
            self.joint_weights = wj.to(dev).contiguous()

        mean = tables.shape_mean_betas if (tables.shape_cov is not None and tables.shape_mean_betas is not None) else None
        self.mean_betas = (torch.zeros(nB) if mean is None else torch.from_numpy(np.asarray(mean, np.float32))[:nB]).to(dev).contiguous()
        self.betas_prec = torch.from_numpy(shape_prior_precision(tables.shape_cov if mean is not None else None, nB)).to(dev).contiguous()
        # parameters: the names and the layout of SMALFitter; the scale tables are one shared (J,3) table each
        self.betas = nn.Parameter(self.mean_betas.clone())
        self.log_beta_scales = nn.Parameter(torch.zeros(J, 3, device=dev), requires_grad=False)
        self.betas_trans = nn.Parameter(torch.zeros(J, 3, device=dev), requires_grad=False)
        self._pose = torch.zeros(N, J, 3, device=dev)
        self._pose[:, 0] = torch.from_numpy(default_global_rotation()).to(dev)
        self.global_rotation = nn.Parameter(self._pose[:, 0])
        self.joint_rotations = nn.Parameter(self._pose[:, 1:])
        self.trans = nn.Parameter(torch.zeros(N, 3, device=dev))
        self.global_mask = torch.ones(1, 3, device=dev)
        self.rotation_mask = torch.ones(J - 1, 3, device=dev)
        self._adam: Dict[str, dict] = {}
        self._adam_hyper = None
        self._adam_step = 0

    # ---- evaluation ------------------------------------------------------------------------------------------
    def _mask_table(self) -> torch.Tensor:
        return torch.cat([self.global_mask.reshape(1, 3), self.rotation_mask.reshape(-1, 3)], 0).float().contiguous()

    def _flags(self) -> dict:
        return dict(propagate_scaling=bool(self.propagate_scaling), allow_limb_scaling=bool(self.config.ALLOW_LIMB_SCALING))

    def _scale_tables(self):
        return self.log_beta_scales.detach().contiguous(), self.betas_trans.detach().contiguous()

    def joints(self) -> torch.Tensor:
        """(N,J,3): the posed joints of the current parameters (fitter convention: ``trans`` added to every joint)."""
        ls, bt = self._scale_tables()
        return engine.joints_forward(self.joint_tables, self.betas.detach().contiguous(), self._pose, self.trans.detach().contiguous(), ls,
                                     bt, self._mask_table(), want_new_J=False, trans_after_joints=True, **self._flags())[0]

    def loss_and_grads(self, w_k3d: float, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0, w_splay: float = 0.0,
                       w_temp: float = 0.0, window: Optional[int] = None):
        """``(objs (10,), grads)``: the loss terms (slots of ``SMIL_N_OBJS``; [9] the 3-D keypoint term) and the gradient of their sum on
        ``betas, pose (N,J,3), trans, log_beta_scales, betas_trans`` - None for a parameter whose ``requires_grad`` is off (``pose``
        holds zero rows for whichever of ``global_rotation`` / ``joint_rotations`` is frozen).  Two launches, no synchronisation."""
        dev, N, J, nB = self.device, self.num_images, self.tables.J, self.n_betas
        window = self.config.WINDOW_SIZE if window is None else int(window)
        train = dict(betas=self.betas.requires_grad and nB > 0, ls=self.log_beta_scales.requires_grad, bt=self.betas_trans.requires_grad)
        cfg = engine.fit_config(N, J, nB, window, (0.0, 0.0, w_betas, w_pose, w_limit, w_splay), w_temp, limit=self.config.JOINT_LIMIT,
                                train_global=self.global_rotation.requires_grad, train_joints=self.joint_rotations.requires_grad,
                                train_trans=self.trans.requires_grad)
        objs = torch.zeros(_lib.N_OBJS, device=dev)
        new = lambda *shape: torch.empty(*shape, device=dev)  # noqa: E731
        d_pose, d_trans = new(N, J, 3), new(N, 3)
        d_betas = torch.zeros(nB, device=dev)  # (zeros: without shape coefficients the kernel writes nothing, the prior adds)
        d_ls, d_bt = (new(J, 3) if train["ls"] else None), (new(J, 3) if train["bt"] else None)
        mask = self._mask_table()
        betas, trans = self.betas.detach().contiguous(), self.trans.detach().contiguous()
        ls, bt = self._scale_tables()
        engine.kp3d_fit_eval(cfg, self.joint_tables, w_k3d, self.robust_scale, self.canonical_joints, self.target_keypoints,
                             self.target_visibility, self.joint_weights, betas, self._pose, trans, ls, bt, mask, objs, d_pose, d_trans,
                             d_betas if train["betas"] else None, d_ls, d_bt, **self._flags())
        engine.prior_losses(cfg, self._pose, trans, betas, self.mean_betas, self.betas_prec, mask, objs, d_pose, d_trans, d_betas,
                            accumulate=True)
        any_pose = self.global_rotation.requires_grad or self.joint_rotations.requires_grad
        grads = dict(betas=d_betas if train["betas"] else None, pose=d_pose if any_pose else None,
                     trans=d_trans if self.trans.requires_grad else None, log_beta_scales=d_ls, betas_trans=d_bt)
        return objs, grads

    # ---- optimiser -------------------------------------------------------------------------------------------
    def begin_stage(self, lr: float, betas=(0.5, 0.999), eps: float = 1e-8):
        """New Adam state per stage, like the reference's new optimiser per stage (optimize_to_joints.py:117-127)."""
        self._adam, self._adam_step = {}, 0
        self._adam_hyper = dict(lr=float(lr), betas=betas, eps=float(eps))

    def fit_step(self, w_k3d: float, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0, w_splay: float = 0.0,
                 w_temp: float = 0.0, window: Optional[int] = None) -> torch.Tensor:
        """One iteration over all frames: losses, gradients and the Adam step of every parameter whose ``requires_grad`` is on
        (optimize_to_joints.py:129-145).  Returns objs (10,) on the device."""
        if self._adam_hyper is None:
            raise RuntimeError("KeypointFitter3D.fit_step: call begin_stage(lr) first")
        objs, grads = self.loss_and_grads(w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp, window)
        h = self._adam_hyper
        self._adam_step += 1
        items = []
        for name, g in grads.items():
            if g is None:
                continue
            p = self._pose if name == "pose" else getattr(self, name).data
            st = self._adam.get(name)
            if st is None:
                st = self._adam[name] = dict(m=torch.zeros_like(p), v=torch.zeros_like(p), t0=self._adam_step - 1)
            items.append((p, g, st["m"], st["v"], h["lr"], self._adam_step - st["t0"]))
        if items:
            # (the bias corrections in double: the float32 ones of smil_adam_step_multi move every parameter by up to 1e-5 of lr per
            # step, which shows on parameters well below 1)
            engine.adam_step_multi_bc64(items, h["betas"][0], h["betas"][1], h["eps"])
        return objs

    # ---- initialisation and export -----------------------------------------------------------------------------
    def initialise_from_alignment(self, min_gap: float = 1e-10) -> torch.Tensor:
        """Rigidly align the joints of the current pose to the visible targets frame by frame (``align.rigid_transform``) and write the
        ``global_rotation`` and ``trans`` that move the model by it (``align.global_pose_from_alignment``).  A frame whose alignment is
        not determined (fewer than three visible targets, collinear ones) keeps its values.  Returns the status (N,) int32."""
        canon = self.canonical_joints.long()
        src = self.joints()[:, canon].contiguous()
        tgt = self.target_keypoints
        seen = torch.isfinite(tgt).all(-1) & (tgt != 0).any(-1)
        if self.target_visibility is not None:
            seen = seen & (self.target_visibility != 0)
        weights = None if self.joint_weights is None else self.joint_weights
        al = _align.rigid_transform(src, tgt, weights=weights, mask=seen, min_gap=min_gap)
        jt = self.joint_tables.host
        root = torch.from_numpy(jt.rest_joints(self.betas.detach().double().cpu().numpy())[0, 0])
        g_old = (self.global_rotation.detach() * self.global_mask).contiguous()
        g_new, t_new = _align.global_pose_from_alignment(None, al.R, al.t, root=root, global_rotation=g_old, trans=self.trans.detach())
        ok = (al.status == _align.OK)[:, None]
        with torch.no_grad():
            self._pose[:, 0] = torch.where(ok, g_new, self._pose[:, 0])
            self.trans.data.copy_(torch.where(ok, t_new, self.trans.data))
        return al.status

    def export_parameters(self, frame_id: int) -> Dict[str, np.ndarray]:
        """The per-frame dict of ``SMALFitter.export_parameters`` without the camera entry."""
        return dict(
            global_rotation=(self.global_rotation.detach()[frame_id] * self.global_mask[0]).cpu().numpy(),
            joint_rotations=(self.joint_rotations.detach()[frame_id] * self.rotation_mask).cpu().numpy(),
            betas=self.betas.detach().cpu().numpy(), trans=self.trans.detach()[frame_id].cpu().numpy(),
            log_betascale=self.log_beta_scales.detach().cpu().numpy(), betas_trans=self.betas_trans.detach().cpu().numpy())
