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

from typing import Optional

import torch

from . import config as _config
from . import engine, model_io
from .fit_keypoints_base import KeypointFitterBase, visibility_table


class KeypointFitter3D(KeypointFitterBase):
    def __init__(self, device, target_keypoints, visibility=None, *, tables: Optional[model_io.SmilModelTables] = None,
                 model_path: Optional[str] = None, config: Optional[_config.FitterConfig] = None, canonical_joints=None,
                 joint_weights=None, robust_scale: float = 0.0):
        super().__init__()
        target = torch.as_tensor(target_keypoints)
        if target.dim() != 3 or target.shape[-1] != 3:
            raise ValueError(f"target_keypoints must be (N,Jc,3), got {tuple(target.shape)}")
        N, Jc = int(target.shape[0]), int(target.shape[1])
        self._init_model(device, N, Jc, tables, model_path, config, canonical_joints, joint_weights)
        self.robust_scale = self._scale(robust_scale, "robust_scale")
        self.target_keypoints = target.to(device=self.device, dtype=torch.float32).contiguous()
        self.target_visibility = visibility_table(visibility, (N, Jc), self.device)

    # ---- evaluation ------------------------------------------------------------------------------------------
    def _term_eval(self, cfg, weights, betas, trans, ls, bt, mask, objs, d_pose, d_trans, d_betas, d_ls, d_bt) -> None:
        engine.kp3d_fit_eval(cfg, self.joint_tables, weights, self.robust_scale, self.canonical_joints, self.target_keypoints,
                             self.target_visibility, self.joint_weights, betas, self._pose, trans, ls, bt, mask, objs, d_pose, d_trans,
                             d_betas, d_ls, d_bt, **self._flags())

    def loss_and_grads(self, w_k3d: float, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0, w_splay: float = 0.0,
                       w_temp: float = 0.0, window: Optional[int] = None):
        """``(objs (10,), grads)``: the loss terms (slots of ``SMIL_N_OBJS``; [9] the 3-D keypoint term) and the gradient of their sum on
        ``betas, pose (N,J,3), trans, log_beta_scales, betas_trans`` - None for a parameter whose ``requires_grad`` is off (``pose``
        holds zero rows for whichever of ``global_rotation`` / ``joint_rotations`` is frozen).  Two launches, no synchronisation."""
        return self._loss_and_grads(w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp, window)

    # ---- optimiser -------------------------------------------------------------------------------------------
    def fit_step(self, w_k3d: float, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0, w_splay: float = 0.0,
                 w_temp: float = 0.0, window: Optional[int] = None) -> torch.Tensor:
        """One iteration over all frames: losses, gradients and the Adam step of every parameter whose ``requires_grad`` is on
        (optimize_to_joints.py:129-145).  Returns objs (10,) on the device."""
        self._require_stage()
        objs, grads = self.loss_and_grads(w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp, window)
        self._adam_apply(grads)
        return objs

    # ---- initialisation ----------------------------------------------------------------------------------------
    def initialise_from_alignment(self, min_gap: float = 1e-10) -> torch.Tensor:
        """Rigidly align the joints of the current pose to the visible targets frame by frame (``align.rigid_transform``) and write the
        ``global_rotation`` and ``trans`` that move the model by it (``align.global_pose_from_alignment``).  A frame whose alignment is
        not determined (fewer than three visible targets, collinear ones) keeps its values.  Returns the status (N,) int32."""
        tgt = self.target_keypoints
        seen = torch.isfinite(tgt).all(-1) & (tgt != 0).any(-1)
        if self.target_visibility is not None:
            seen = seen & (self.target_visibility != 0)
        return self._initialise_from_alignment(tgt, seen, min_gap)
