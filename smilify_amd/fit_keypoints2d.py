"""Sequence fitter for multi-view 2-D keypoint detections: the model's posed joints, projected into every calibrated view, against the
detections themselves - no mesh, no renderer and no triangulation in between.

``KeypointFitter2D`` holds the parameters of ``SMALFitter`` under the same names and fits them to ``target_keypoints_2d (N,Nv,Jc,2)`` in
``(y, x)`` pixels of an ``image_size`` x ``image_size`` image (the order of ``SMALFitter.target_joints``).  An iteration is three launches,
as in ``KeypointFitter3D``: ``smil_kp2d_fit_eval`` (chain, joints, projection, the term and its backward of every frame in one kernel,
csrc/joints.hip), ``smil_prior_losses(accumulate=1)`` and ``smil_adam_step_multi_bc64``.  Nothing synchronises the host.  The term
(objs[0]; windows as in ``SMALFitter``; image ``frame * views + view``):

    w_k2d sum_w 1/(2 Jc Nv b_w) sum_{n in w} sum_v sum_c seen[n,v,c] conf[n,v,c] wj[c] rho(|yx(joints[n,canon[c]]; cam(n,v)) - target[n,v,c]|^2)

``rho(s) = s`` - then, without confidences and joint weights, it is the joint loss of ``SMALFitter`` (fitter.py:292-296) summed over the
views in the fitter's own normalisation, so the reference's stage weights carry over - or the soft-L1
``2 sigma^2 (sqrt(1 + s / sigma^2) - 1)`` with ``robust_scale_px = sigma > 0``.  An entry is seen iff its visibility (if given) is
non-zero, both target coordinates are finite, its confidence (if given) is finite and > 0, and the joint lies more than the near plane
(0.001) in front of that camera.  With ``target_keypoints_3d`` the 3-D term of ``KeypointFitter3D`` (objs[9]) can be asked for in the same
launch (``w_k3d > 0``).

Cameras: a ``cameras.FoVCameras`` or a dict with ``R``, ``T``, ``fov`` (degrees) and optionally ``aspect_ratio`` and ``principal_point``
(NDC); every table holds 1, ``views`` or ``N * views`` rows and is indexed ``image % rows``.  ``cameras.opencv_to_pinhole_camera(R_cv, t_cv,
K, S)`` returns such a camera for an OpenCV calibration; for ANY ``S`` it reproduces ``u = fx x / z + cx``, ``v = fy y / z + cy`` exactly, so
keypoints in full, non-square camera frames need no crop: pick ``S`` and pass it as ``image_size``.

Not supported: gradients on the cameras or ``fov`` (they are constants of this fit); more than 64 views; models with pose blend shapes
(``joints.JointTables`` raises); per-frame scale tables (``log_beta_scales`` and ``betas_trans`` are one shared (J,3) table each); several
ranks; hipGraph capture of the step; a command-line driver.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from . import config as _config
from . import engine, model_io
from .cameras import FoVCameras
from .fit_keypoints_base import KeypointFitterBase, visibility_table

MAX_VIEWS = 64


def _camera_set(cameras, views: int, N: int, S: int, device) -> engine.CameraSet:
    """The device ``CameraSet`` of a ``FoVCameras`` or a dict; every table has 1, ``views`` or ``N * views`` rows."""
    if isinstance(cameras, FoVCameras):
        cameras = dict(R=cameras.R, T=cameras.T, fov=cameras.fov, aspect_ratio=cameras.aspect_ratio, principal_point=cameras.principal_point)
    if not isinstance(cameras, dict) or any(k not in cameras for k in ("R", "T", "fov")):
        raise ValueError("cameras must be a cameras.FoVCameras or a dict holding R, T and fov (optional: aspect_ratio, principal_point)")
    unknown = set(cameras) - {"R", "T", "fov", "aspect_ratio", "principal_point"}
    if unknown:
        raise ValueError(f"cameras holds unknown entries {sorted(unknown)}")

    def table(name, tail):
        t = cameras.get(name)
        if t is None:
            return None
        t = torch.as_tensor(t).detach().to(device=device, dtype=torch.float32)
        t = t.reshape(-1, *tail) if t.dim() <= len(tail) else t
        if tuple(t.shape[1:]) != tail:
            raise ValueError(f"camera table {name} must be (k,{','.join(map(str, tail))}), got {tuple(t.shape)}" if tail else
                             f"camera table {name} must be (k,), got {tuple(t.shape)}")
        if t.shape[0] not in (1, views, N * views):
            raise _lib.SmilError(f"camera table {name} has {t.shape[0]} rows; expected 1, views={views} or N*views={N * views}")
        return t.contiguous()

    return engine.CameraSet(R=table("R", (3, 3)), T=table("T", (3,)), fov=table("fov", ()), aspect=table("aspect_ratio", ()), views=views, S=S,
                            principal=table("principal_point", (2,)))


class KeypointFitter2D(KeypointFitterBase):
    def __init__(self, device, target_keypoints_2d, visibility=None, *, cameras, image_size: int, confidence=None,
                 target_keypoints_3d=None, visibility_3d=None, tables: Optional[model_io.SmilModelTables] = None,
                 model_path: Optional[str] = None, config: Optional[_config.FitterConfig] = None, canonical_joints=None,
                 joint_weights=None, robust_scale_px: float = 0.0, robust_scale: float = 0.0):
        super().__init__()
        target = torch.as_tensor(target_keypoints_2d)
        if target.dim() != 4 or target.shape[-1] != 2:
            raise ValueError(f"target_keypoints_2d must be (N,Nv,Jc,2), got {tuple(target.shape)}")
        N, Nv, Jc = (int(s) for s in target.shape[:3])
        if not 1 <= Nv <= MAX_VIEWS:
            raise _lib.SmilError(f"KeypointFitter2D: views={Nv} outside 1..{MAX_VIEWS}")
        if int(image_size) != image_size or int(image_size) < 1:
            raise ValueError(f"image_size must be a positive integer, got {image_size}")
        self._init_model(device, N, Jc, tables, model_path, config, canonical_joints, joint_weights)
        dev = self.device
        self.views, self.image_size = Nv, int(image_size)
        self.robust_scale_px = self._scale(robust_scale_px, "robust_scale_px")
        self.robust_scale = self._scale(robust_scale, "robust_scale")
        self.cameras = _camera_set(cameras, Nv, N, self.image_size, dev)
        self.target_keypoints_2d = target.to(device=dev, dtype=torch.float32).contiguous()
        self.target_visibility = visibility_table(visibility, (N, Nv, Jc), dev)
        self.confidence = None
        if confidence is not None:
            conf = torch.as_tensor(confidence)
            if tuple(conf.shape) != (N, Nv, Jc):
                raise ValueError(f"confidence must be ({N},{Nv},{Jc}), got {tuple(conf.shape)}")
            self.confidence = conf.to(device=dev, dtype=torch.float32).contiguous()
        self.target_keypoints_3d = self.target_visibility_3d = None
        if target_keypoints_3d is not None:
            t3 = torch.as_tensor(target_keypoints_3d)
            if tuple(t3.shape) != (N, Jc, 3):
                raise ValueError(f"target_keypoints_3d must be ({N},{Jc},3), got {tuple(t3.shape)}")
            self.target_keypoints_3d = t3.to(device=dev, dtype=torch.float32).contiguous()
            self.target_visibility_3d = visibility_table(visibility_3d, (N, Jc), dev, "visibility_3d")
        elif visibility_3d is not None:
            raise ValueError("visibility_3d without target_keypoints_3d")

    # ---- evaluation ------------------------------------------------------------------------------------------
    def _term_eval(self, cfg, weights, betas, trans, ls, bt, mask, objs, d_pose, d_trans, d_betas, d_ls, d_bt, yx_out=None,
                   joints_out=None) -> None:
        w_k2d, w_k3d = weights
        engine.kp2d_fit_eval(cfg, self.joint_tables, self.cameras, w_k2d, self.robust_scale_px, self.canonical_joints,
                             self.target_keypoints_2d, self.target_visibility, self.confidence, self.joint_weights, betas, self._pose, trans,
                             ls, bt, mask, objs, d_pose, d_trans, d_betas, d_ls, d_bt, yx_out=yx_out, joints_out=joints_out, w_k3d=w_k3d,
                             robust_scale=self.robust_scale, target3d=self.target_keypoints_3d, visibility3d=self.target_visibility_3d,
                             **self._flags())

    def loss_and_grads(self, w_k2d: float, w_k3d: float = 0.0, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0,
                       w_splay: float = 0.0, w_temp: float = 0.0, window: Optional[int] = None):
        """``(objs (10,), grads)``: the loss terms (slots of ``SMIL_N_OBJS``; [0] the 2-D keypoint term, [9] the 3-D one) and the gradient
        of their sum on ``betas, pose (N,J,3), trans, log_beta_scales, betas_trans`` - None for a parameter whose ``requires_grad`` is off.
        Two launches, no synchronisation.  ``w_k3d > 0`` needs ``target_keypoints_3d``."""
        if w_k3d > 0 and self.target_keypoints_3d is None:
            raise ValueError("KeypointFitter2D: w_k3d > 0 but no target_keypoints_3d were given")
        return self._loss_and_grads((w_k2d, w_k3d), w_betas, w_pose, w_limit, w_splay, w_temp, window)

    def project(self, return_joints: bool = False):
        """(N,Nv,Jc,2) float32: the ``(y, x)`` pixel positions of the canonical joints of the current parameters in every view (the kernel's
        ``yx_out``); NaN where a joint is not in front of the camera's near plane.  A diagnostic, not part of an iteration: it is one
        launch of the whole fused kernel (chain forward, term, reverse walk with no gradient output asked for).  ``return_joints``: also the
        kernel's ``joints_out (N,J,3)``, the posed joints it projected."""
        N, J, nB = self.num_images, self.tables.J, self.n_betas
        cfg = engine.fit_config(N, J, nB, 0, (0.0,) * 6, 0.0, limit=self.config.JOINT_LIMIT)
        yx = torch.empty(N, self.views, int(self.canonical_joints.numel()), 2, device=self.device)
        ls, bt = self._scale_tables()
        objs = torch.zeros(_lib.N_OBJS, device=self.device)
        joints = torch.empty(N, J, 3, device=self.device) if return_joints else None
        self._term_eval(cfg, (1.0, 0.0), self.betas.detach().contiguous(), self.trans.detach().contiguous(), ls, bt, self._mask_table(), objs,
                        None, None, None, None, None, yx_out=yx, joints_out=joints)
        return (yx, joints) if return_joints else yx

    def seen(self) -> torch.Tensor:
        """(N,Nv,Jc) bool: the entries the term sees at the current parameters (one ``project()``)."""
        return self._seen(self.project())

    def _seen(self, yx) -> torch.Tensor:
        seen = torch.isfinite(self.target_keypoints_2d).all(-1) & torch.isfinite(yx).all(-1)
        if self.target_visibility is not None:
            seen = seen & (self.target_visibility != 0)
        if self.confidence is not None:
            seen = seen & torch.isfinite(self.confidence) & (self.confidence > 0)
        return seen

    def reprojection_errors(self) -> torch.Tensor:
        """(N,Nv,Jc) float32: the pixel distance of every projected joint from its target, NaN where the entry is not seen (one
        ``project()``)."""
        yx = self.project()
        dist = (yx - self.target_keypoints_2d).norm(dim=-1)
        return torch.where(self._seen(yx), dist, torch.full_like(dist, float("nan")))

    # ---- optimiser -------------------------------------------------------------------------------------------
    def fit_step(self, w_k2d: float, w_k3d: float = 0.0, w_betas: float = 0.0, w_pose: float = 0.0, w_limit: float = 0.0,
                 w_splay: float = 0.0, w_temp: float = 0.0, window: Optional[int] = None) -> torch.Tensor:
        """One iteration over all frames: losses, gradients and the Adam step of every parameter whose ``requires_grad`` is on.  Returns
        objs (10,) on the device."""
        self._require_stage()
        objs, grads = self.loss_and_grads(w_k2d, w_k3d, w_betas, w_pose, w_limit, w_splay, w_temp, window)
        self._adam_apply(grads)
        return objs

    # ---- initialisation ----------------------------------------------------------------------------------------
    def initialise_from_alignment(self, min_gap: float = 1e-10) -> torch.Tensor:
        """``KeypointFitter3D.initialise_from_alignment`` on the 3-D targets; raises when none were given (2-D detections alone determine
        no rigid alignment)."""
        tgt = self.target_keypoints_3d
        if tgt is None:
            raise RuntimeError("KeypointFitter2D.initialise_from_alignment needs target_keypoints_3d: 2-D detections alone determine no "
                               "rigid 3-D alignment (triangulate them first, or start from the default pose)")
        seen = torch.isfinite(tgt).all(-1) & (tgt != 0).any(-1)
        if self.target_visibility_3d is not None:
            seen = seen & (self.target_visibility_3d != 0)
        return self._initialise_from_alignment(tgt, seen, min_gap)
