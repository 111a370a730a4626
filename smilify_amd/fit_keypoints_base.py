"""What the mesh-free keypoint fitters share (``KeypointFitter3D``, ``KeypointFitter2D``): the model tables and the parameters of
``SMALFitter`` under the same names, the mask table, the finishing ``smil_prior_losses`` launch, the Adam bookkeeping and the export.
A subclass supplies ``_term_eval`` - the one launch that adds its terms into ``objs`` and writes the RAW gradients."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import config as _config
from . import engine, model_io
from .fitter import default_global_rotation, shape_prior_precision
from .joints import JointTables


def visibility_table(visibility, shape, device, name="visibility") -> Optional[torch.Tensor]:
    """None, or the uint8 table (non-zero -> 1) of ``shape`` on the device."""
    if visibility is None:
        return None
    vis = torch.as_tensor(visibility)
    if tuple(vis.shape) != tuple(shape):
        raise ValueError(f"{name} must be ({','.join(str(s) for s in shape)}), got {tuple(vis.shape)}")
    return (vis != 0).to(device=device, dtype=torch.uint8).contiguous()


class KeypointFitterBase(nn.Module):
    def _init_model(self, device, N: int, Jc: int, tables, model_path, config, canonical_joints, joint_weights):
        """Tables, the canonical joint list, the joint weights and the parameters of an N-frame fit to Jc keypoints."""
        who = type(self).__name__
        self.device = dev = engine.require_gpu(device)
        if tables is None:
            cfg0 = config or _config.current
            path = model_path or (cfg0.SMAL_FILE if cfg0 is not None else None)
            if path is None:
                raise ValueError(f"{who} needs tables=, model_path= or config.SMAL_FILE")
            tables = model_io.load_model(path)
        self.tables = tables
        self.config = cfg = config or _config.current or _config.FitterConfig.from_tables(tables, model_path)
        self.joint_tables = engine.DeviceJointTables(JointTables.from_tables(tables), dev)
        J, nB = tables.J, tables.nB
        canon = list(cfg.CANONICAL_MODEL_JOINTS if canonical_joints is None else canonical_joints)
        if len(canon) != Jc or any(not 0 <= int(c) < J for c in canon):
            raise ValueError(f"canonical_joints must name {Jc} joints of 0..{J - 1}, got {canon}")
        self.num_images, self.n_betas = N, nB
        self.propagate_scaling = False
        self.canonical_joints = torch.tensor(canon, dtype=torch.int32, device=dev)
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

    @staticmethod
    def _scale(value, name: str) -> float:
        value = float(value)
        if not np.isfinite(value) or value < 0:
            raise ValueError(f"{name} must be finite and not negative, got {value}")
        return value

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

    def _term_eval(self, cfg, weights, betas, trans, ls, bt, mask, objs, d_pose, d_trans, d_betas, d_ls, d_bt) -> None:
        raise NotImplementedError

    def _loss_and_grads(self, term_weights, w_betas, w_pose, w_limit, w_splay, w_temp, window):
        """``_term_eval(term_weights)`` then ``smil_prior_losses(accumulate=1)``: two launches, no synchronisation."""
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
        self._term_eval(cfg, term_weights, betas, trans, ls, bt, mask, objs, d_pose, d_trans, d_betas if train["betas"] else None, d_ls, d_bt)
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

    def _require_stage(self):
        if self._adam_hyper is None:
            raise RuntimeError(f"{type(self).__name__}.fit_step: call begin_stage(lr) first")

    def _adam_apply(self, grads) -> None:
        """The Adam step of every parameter that has a gradient: one launch."""
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

    # ---- initialisation and export -----------------------------------------------------------------------------
    def _initialise_from_alignment(self, tgt, seen, min_gap: float) -> torch.Tensor:
        """Rigid alignment of the current joints to the 3-D targets ``tgt (N,Jc,3)`` where ``seen``, written into ``global_rotation`` and
        ``trans``; returns the status (N,) int32."""
        from . import align as _align

        canon = self.canonical_joints.long()
        src = self.joints()[:, canon].contiguous()
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
