"""Thin torch-tensor front end over the C ABI (include/smilfit.h).

PyTorch is used for device memory, streams and autograd plumbing only; every arithmetic step of the hot
path is a HIP kernel inside ``libsmilfit.so``.  All functions launch on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .model_io import SmilModelTables

# Renderer settings of the reference (smal_fitter/p3d_renderer.py:24-25,41-47)
SIGMA = 1e-4
BLUR_RADIUS = float(np.log(1.0 / 1e-4 - 1.0) * 1e-4)
FACES_PER_PIXEL = 100
ZNEAR, ZFAR = 0.001, 1000.0


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Caller-owned scratch of the size a ``smil_*_workspace_bytes`` query returned."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _f32(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def require_gpu(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SmilError(f"smilify_amd runs on an AMD GPU only (got device '{device}'); there is no CPU path")
    if not torch.cuda.is_available():
        raise _lib.SmilError("no GPU visible to PyTorch-ROCm; smilify_amd has no CPU fallback")
    return device


_SHARED_WS: Dict = {}  # (device type, index) -> the device's rasteriser workspace
_WS_USER: Dict = {}    # (device type, index) -> (model, stream) of the most recent rasteriser call in that workspace


class DeviceModel:
    """Model constants resident on one GPU (``SmilModel*``)."""

    def __init__(self, tables: SmilModelTables, device):
        self.device = require_gpu(device)
        self.tables = tables
        lib = _lib.checked()
        t = tables
        arrs = dict(
            v_template=np.ascontiguousarray(t.v_template, np.float32),
            shapedirs=np.ascontiguousarray(t.shapedirs, np.float32),
            faces=np.ascontiguousarray(t.faces, np.int32),
            parents=np.ascontiguousarray(t.parents, np.int32),
            skin_idx=np.ascontiguousarray(t.skin_idx, np.int32),
            skin_w=np.ascontiguousarray(t.skin_w, np.float32),
            jreg_rowptr=np.ascontiguousarray(t.jreg_rowptr, np.int32),
            jreg_col=np.ascontiguousarray(t.jreg_col, np.int32),
            jreg_val=np.ascontiguousarray(t.jreg_val, np.float32),
        )
        if t.static_joints:
            arrs["J_static"] = np.ascontiguousarray(t.J_static, np.float32)
        if t.posedirs is not None:
            if t.posedirs.shape != (9 * (t.J - 1), 3 * t.V):
                raise _lib.SmilError(f"posedirs shape {t.posedirs.shape} != ({9 * (t.J - 1)}, {3 * t.V})")
            arrs["posedirs"] = np.ascontiguousarray(t.posedirs, np.float32)
        d = _lib.ModelDesc()
        d.V, d.F, d.J, d.nB = t.V, t.F, t.J, t.nB
        for k, a in arrs.items():
            setattr(d, k, a.ctypes.data if a.size else None)
        d.static_joints = 1 if t.static_joints else 0
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            lib.smil_model_create(ctypes.byref(d), ctypes.byref(handle))
        self.handle = handle
        self.V, self.F, self.J, self.nB = t.V, t.F, t.J, t.nB
        self.static_joints = bool(t.static_joints)
        self.has_posedirs = t.posedirs is not None
        self._ws: Optional[torch.Tensor] = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().smil_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def faces_i32(self) -> torch.Tensor:
        """The face table as an int32 device tensor (lazily uploaded copy of what smil_model_create received)."""
        if getattr(self, "_faces_dev", None) is None:
            self._faces_dev = torch.from_numpy(np.ascontiguousarray(self.tables.faces, np.int32)).to(self.device)
        return self._faces_dev

    def _ws_key(self):
        return (self.device.type, self.device.index if self.device.index is not None else torch.cuda.current_device())

    def workspace(self, N: int, S: int) -> torch.Tensor:
        """Rasteriser workspace: ONE buffer per device, shared by every model and topology on it (most of it is the scratch
        arena of the resident workgroups, whatever the mesh), grown when a call needs more; every model then points at the
        grown buffer (a captured hipGraph holds the tensor it was captured with itself, ``fit_graph.capture``).
        Every call rewrites what it reads, so models may take turns - in STREAM ORDER: a call on another stream than the
        previous one first waits for everything submitted to that stream (``_claim_workspace``)."""
        need = int(_lib.load().smil_raster_workspace_bytes(self.handle, N, S))
        key = self._ws_key()
        ws = _SHARED_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _SHARED_WS[key] = _workspace(need, self.device)
        self._ws = ws
        return ws

    def _claim_workspace(self) -> None:
        """Book-keeping of a rasteriser call about to be launched: order it behind the previous user of the shared workspace when that
        one ran on another stream, and remember who used the workspace last (``raster_stats``)."""
        key = self._ws_key()
        cur = torch.cuda.current_stream(self.device)
        prev = _WS_USER.get(key)
        if prev is not None and prev[1] != cur and not torch.cuda.is_current_stream_capturing():
            cur.wait_stream(prev[1])
        _WS_USER[key] = (self, cur)


@dataclass
class CameraSet:
    """FoV-perspective cameras; tables with k rows are indexed ``image % k`` (k = 1, views or N).  With ``principal`` (k,2), the
    principal point ``(px, py)`` in NDC, they are pytorch3d's ``PerspectiveCameras``: ``x_ndc = K00 x / z + px`` (None: centred).  The
    table is a constant: it carries no gradient."""

    R: torch.Tensor  # (nR,3,3)
    T: torch.Tensor  # (nT,3)
    fov: torch.Tensor  # (nFov,) degrees
    aspect: Optional[torch.Tensor]
    views: int
    S: int
    principal: Optional[torch.Tensor] = None  # (nPrincipal,2) float32, contiguous

    def struct(self, N: int) -> _lib.Cameras:
        c = _lib.Cameras()
        c.N, c.views, c.S = N, self.views, self.S
        c.R, c.nR = self.R.data_ptr(), self.R.shape[0]
        c.T, c.nT = self.T.data_ptr(), self.T.shape[0]
        c.fov, c.nFov = self.fov.data_ptr(), self.fov.numel()
        if self.aspect is not None:
            c.aspect, c.nAspect = self.aspect.data_ptr(), self.aspect.numel()
        else:
            c.aspect, c.nAspect = None, 0
        tables = [("R", c.nR), ("T", c.nT), ("fov", c.nFov)]
        if self.principal is not None:
            pp = self.principal
            if pp.requires_grad:
                raise NotImplementedError("the principal point carries no gradient: pass a tensor that does not require one")
            if pp.dim() != 2 or pp.shape[1] != 2 or pp.dtype != torch.float32 or not pp.is_contiguous():
                raise _lib.SmilError(f"camera table principal must be a contiguous float32 (k,2) tensor, got {tuple(pp.shape)} {pp.dtype}")
            c.principal, c.nPrincipal = pp.data_ptr(), pp.shape[0]
            tables.append(("principal", c.nPrincipal))
        else:
            c.principal, c.nPrincipal = None, 0
        for name, k in tables:
            if k not in (1, self.views, N):
                raise _lib.SmilError(f"camera table {name} has {k} rows; expected 1, views={self.views} or N={N}")
        return c


TIE_RULES = {"depth_face_id": _lib.TIE_DEPTH_FACE_ID, "reference_queue": _lib.TIE_REFERENCE_QUEUE}


class ClipDepth:
    """Caller-owned buffers of the rasteriser's depth-gradient side channel (``SmilClipDepth``): the end points of edges that
    cross the clipping plane receive a gradient on their DEPTH (pytorch3d differentiates ``clip_faces`` through its
    interpolation weight), which ``d_ndc (N,V,2)`` cannot hold.  ``silhouette_backward`` / ``silhouette_l1_fused`` fill it
    (``clip_depth=``), ``lbs_backward(ndc_upstream=dict(..., clip_depth=))`` or ``clip_depth_backward`` consume it."""

    def __init__(self, device, n_images: int, capacity: int = 1 << 18):
        dev = torch.device(device)
        self.n_images, self.capacity = int(n_images), int(capacity)
        self.vertex = torch.empty(capacity, dtype=torch.int32, device=dev)  # (entries are written before they are read: range / counter say which)
        self.dz = torch.empty(capacity, dtype=torch.float32, device=dev)
        self.range = torch.zeros(n_images, 2, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(2, dtype=torch.int32, device=dev)
        self._struct = _lib.ClipDepth(self.vertex.data_ptr(), self.dz.data_ptr(), self.range.data_ptr(), self.counter.data_ptr(), self.capacity)

    def pointer(self):
        return ctypes.cast(ctypes.pointer(self._struct), ctypes.c_void_p)

    def dense(self, V: int) -> torch.Tensor:
        """(n_images, V) depth gradients (tests; synchronises)."""
        out = torch.zeros(self.n_images, V, dtype=torch.float64)
        rg, vx, dz = self.range.cpu().numpy(), self.vertex.cpu().numpy(), self.dz.cpu().numpy()
        for n in range(self.n_images):
            for e in range(int(rg[n, 0]), int(rg[n, 0]) + int(rg[n, 1])):
                out[n, int(vx[e])] += float(dz[e])
        return out


def clip_depth_for(model: "DeviceModel", n_images: int) -> ClipDepth:
    """The model's cached ``ClipDepth`` for calls of ``n_images`` images (one per size: a captured graph keeps its pointers).
    The cache is shared by every fitter, renderer and stream that uses this ``DeviceModel``: correctness relies on the produce
    (rasteriser call) -> consume (LBS / projection backward) pair of one evaluation being issued back to back on ONE stream, as
    ``SMALFitter._loss_and_grads`` does; callers that interleave evaluations of the same size on several streams must bring their own
    ``ClipDepth``."""
    cache = model.__dict__.setdefault("_clip_depth_cache", {})
    if n_images not in cache:
        cache[n_images] = ClipDepth(model.device, n_images)
    return cache[n_images]


def _rs_for_slice(rs, clip_depth: Optional["ClipDepth"], image0: int):
    """A copy of the raster settings that names the depth-gradient sink and the slice's first image."""
    if clip_depth is None:
        return rs
    cp = _lib.RasterSettings()
    ctypes.pointer(cp)[0] = rs
    cp.clip_depth, cp.image0 = clip_depth.pointer(), int(image0)
    return cp


def clip_depth_backward(cams: "CameraSet", clip_depth: ClipDepth, d_verts: torch.Tensor) -> None:
    """``d_verts`` (frames,V,3) += the depth gradients of ``clip_depth`` carried through the cameras (separate-kernel route)."""
    N = d_verts.shape[0] * cams.views
    c = cams.struct(N)
    _lib.checked().smil_clip_depth_backward(ctypes.byref(c), ctypes.byref(clip_depth._struct), N, d_verts.shape[1], _ptr(d_verts), _stream())


def raster_settings(blur=BLUR_RADIUS, sigma=SIGMA, K=FACES_PER_PIXEL, tie_rule="depth_face_id") -> _lib.RasterSettings:
    """``tie_rule``: which faces a truncated pixel keeps among equal depths at its K-th place - ``"depth_face_id"`` (default: the
    smallest face ids, order independent) or ``"reference_queue"`` (what pytorch3d's unsorted K-queue keeps when it visits the
    faces in index order, the reference's rasteriser: those pixels are replayed by a second kernel)."""
    rs = _lib.RasterSettings()
    rs.blur_radius, rs.sigma, rs.faces_per_pixel, rs.z_clip = blur, sigma, K, ZNEAR / 2
    rs.tie_rule = TIE_RULES[tie_rule] if isinstance(tie_rule, str) else int(tie_rule)
    return rs


# ----------------------------------------------------------------------------------------------
# LBS
# ----------------------------------------------------------------------------------------------
def _lbs_inputs(inp: Dict, fl: Dict) -> _lib.LbsInputs:
    """The ``LbsInputs`` struct of a call: its input tensors and its flags, as ``lbs_forward`` saves them for ``lbs_backward``."""
    i = _lib.LbsInputs()
    for k, v in fl.items():
        setattr(i, k, int(v))
    for k, t in inp.items():
        setattr(i, k, None if t is None else t.data_ptr())
    return i


def lbs_forward(model: DeviceModel, beta, theta, trans=None, logscale=None, btrans=None, del_v=None,
                v_template=None, Rs_in=None, shared_beta=False, logscale_shared=False, btrans_shared=False,
                propagate_scaling=False, allow_limb_scaling=True, trans_after_joints=False, theta_mask=None,
                project: Optional[Dict] = None) -> Dict[str, torch.Tensor]:
    """``theta_mask`` (J,3): the kernels use ``theta * mask`` without a masked copy being made (SMALFitter's rotation masks);
    ``lbs_backward`` then returns ``d_theta`` as the gradient on ``theta * mask`` (``fit_epilogue`` multiplies it by the mask).
    ``project`` = ``dict(cams=CameraSet, ndc=bool, yx=bool)``: the vertices / joints are also projected through the cameras
    (``smil_lbs_forward_project``: one kernel per frame with skinning and joint regression); the result carries ``ndc`` (N,V,3)
    and / or ``yx`` (N,J,2)."""
    dev = model.device
    B = int((theta if theta is not None else Rs_in).shape[0])
    J, V = model.J, model.V
    nB_used = int(beta.shape[-1])
    nS = 1 if (shared_beta and del_v is None) else B
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = dict(v_shaped=f(nS, V, 3), J_rest=f(nS, J, 3), Rs=f(B, J, 3, 3), G=f(B, J, 3, 4), A=f(B, J, 3, 4),
               new_J=f(B, J, 3), verts=f(B, V, 3), joints=f(B, J, 3))
    if model.has_posedirs:
        out["v_posed"] = f(B, V, 3)
    inp = dict(beta=beta, theta=theta, Rs_in=Rs_in, logscale=logscale, btrans=btrans, trans=trans, del_v=del_v,
               v_template=v_template, theta_mask=theta_mask)
    fl = dict(B=B, shared_beta=shared_beta, nB_used=nB_used, logscale_shared=logscale_shared, btrans_shared=btrans_shared,
              propagate_scaling=propagate_scaling, allow_limb_scaling=allow_limb_scaling, trans_after_joints=trans_after_joints)
    i = _lbs_inputs(inp, fl)
    o = _lib.LbsOutputs()
    for k, t in out.items():
        setattr(o, k, t.data_ptr())
    ndc = yx = None
    if project is not None:
        cams = project["cams"]
        N = B * cams.views
        ndc = f(N, V, 3) if project.get("ndc", True) else None
        yx = f(N, J, 2) if project.get("yx", True) else None
        c = cams.struct(N)
        _lib.checked().smil_lbs_forward_project(model.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(c), _ptr(ndc), _ptr(yx), _stream())
    else:
        _lib.checked().smil_lbs_forward(model.handle, ctypes.byref(i), ctypes.byref(o), _stream())
    if ndc is not None:
        out["ndc"] = ndc
    if yx is not None:
        out["yx"] = yx
    out["_inputs"] = inp
    out["_flags"] = fl
    return out


# SMILFIT_UNFUSED_LBS=1 (A/B measurements, tools/dbg/ab_lbs.sh): the fit iteration takes the separate projection / skinning kernels
FUSED_LBS_FORWARD = os.environ.get("SMILFIT_UNFUSED_LBS") != "1"   # projection inside the skinning kernel (smil_lbs_forward_project)
FUSED_LBS_BACKWARD = os.environ.get("SMILFIT_UNFUSED_LBS") != "1"  # the fit iteration takes smil_lbs_backward_ndc where the library supports the model (tests switch it off to compare)


def lbs_backward_ndc_supported(model: DeviceModel, nB_used: int, views: int) -> bool:
    """Whether ``lbs_backward(..., ndc_upstream=...)`` (one kernel from the image plane) handles this model and call."""
    # a predicate, not a status: asked of the raw library, where a non-zero answer raises nothing
    return bool(_lib.load().smil_lbs_backward_ndc_supported(model.handle, int(nB_used), int(views)))


def lbs_backward(model: DeviceModel, saved: Dict, d_verts, d_joints, need_beta=True, need_theta=True,
                 need_logscale=True, need_btrans=True, need_trans=True, need_vshaped=False,
                 need_Rs=False, d_beta_accum: Optional[torch.Tensor] = None, out_logscale: Optional[torch.Tensor] = None,
                 out_btrans: Optional[torch.Tensor] = None, ndc_upstream: Optional[Dict] = None, up_Rs: Optional[torch.Tensor] = None,
                 up_v_shaped: Optional[torch.Tensor] = None) -> Dict[str, Optional[torch.Tensor]]:
    """``d_beta_accum`` (shared betas only): the sum over frames is ADDED to this (nB,) tensor instead of a fresh one.
    ``out_logscale`` / ``out_btrans`` (shared tables only): (J,3) buffers that receive those gradients (overwritten).
    ``ndc_upstream`` = ``dict(cams=CameraSet, d_ndc=, d_ndc_scale=, d_yx=, d_fov_img=)`` instead of ``d_verts`` / ``d_joints``:
    the gradients are taken on the image plane and projected back inside the skinning backward (``smil_lbs_backward_ndc``);
    the result then carries ``d_joints`` (B,J,3).
    ``up_Rs`` (B,J,3,3) / ``up_v_shaped`` (nS,V,3): upstream gradients on the returned rotation matrices / shaped vertices."""
    dev = model.device
    inp, fl = saved["_inputs"], saved["_flags"]
    B, J = fl["B"], model.J
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    g = dict(d_beta=None, d_theta=None, d_logscale=None, d_btrans=None, d_trans=None, d_del_v=None, d_Rs_in=None)
    if need_vshaped:  # per-frame gradient on v_shaped = on del_v (and, summed over frames, on a custom v_template)
        g["d_del_v"] = f(B, model.V, 3)
    if need_Rs and inp["Rs_in"] is not None:
        g["d_Rs_in"] = f(B, J, 3, 3)
    accumulate_beta = False
    if need_beta and fl["nB_used"] > 0:
        if fl["shared_beta"] and d_beta_accum is not None:
            g["d_beta"], accumulate_beta = d_beta_accum, True
        else:
            g["d_beta"] = f(fl["nB_used"]) if fl["shared_beta"] else f(B, fl["nB_used"])
    if need_theta and inp["theta"] is not None:
        g["d_theta"] = f(B, J, 3)
    if need_logscale and inp["logscale"] is not None and fl["allow_limb_scaling"]:
        g["d_logscale"] = (out_logscale if out_logscale is not None else f(J, 3)) if fl["logscale_shared"] else f(B, J, 3)
    if need_btrans and inp["btrans"] is not None:
        g["d_btrans"] = (out_btrans if out_btrans is not None else f(J, 3)) if fl["btrans_shared"] else f(B, J, 3)
    if need_trans:
        g["d_trans"] = f(B, 3)
    scratch = dict(d_A=f(B, J, 12), d_Jrest=f(B, J, 3), d_Rs=f(B, J, 9))
    if g["d_beta"] is not None and fl["shared_beta"]:
        scratch["beta_rows"] = f(2 * B * fl["nB_used"] + 16)  # per-block partial sums of the shared shape gradient (added in a fixed order) + the call's block counter
    i = _lbs_inputs(inp, fl)
    o = _lib.LbsOutputs()
    for k in ("v_shaped", "J_rest", "Rs", "G", "A", "new_J", "verts", "joints"):
        setattr(o, k, saved[k].data_ptr())
    if model.has_posedirs:
        o.v_posed = saved["v_posed"].data_ptr()
        scratch["d_vposed"] = f(B, model.V, 3)
        scratch["d_posefeat"] = f(B, 9 * (J - 1))
    gs = _lib.LbsGrads()
    gs.d_verts = None if d_verts is None else d_verts.data_ptr()
    gs.d_joints = None if d_joints is None else d_joints.data_ptr()
    for k, t in {**g, **scratch}.items():
        setattr(gs, k, None if t is None else t.data_ptr())
    gs.accumulate_shared_beta = int(accumulate_beta)
    gs.up_Rs = None if up_Rs is None else up_Rs.data_ptr()
    gs.up_v_shaped = None if up_v_shaped is None else up_v_shaped.data_ptr()
    if ndc_upstream is not None:
        if d_verts is not None or d_joints is not None or need_vshaped:
            raise ValueError("ndc_upstream replaces d_verts / d_joints and has no del_v gradient")
        up = ndc_upstream
        cams = up["cams"]
        g["d_joints"] = f(B, J, 3)
        if up.get("clip_depth") is not None:
            gs.clip_depth = up["clip_depth"].pointer()
        c = cams.struct(B * cams.views)
        _lib.checked().smil_lbs_backward_ndc(model.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(gs), ctypes.byref(c), _ptr(up.get("d_ndc")),
                                             _ptr(up.get("d_ndc_scale")), _ptr(up.get("d_yx")), _ptr(g["d_joints"]), _ptr(up.get("d_fov_img")),
                                             _stream())
        return g
    _lib.checked().smil_lbs_backward(model.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(gs), _stream())
    return g


# ----------------------------------------------------------------------------------------------
# projection
# ----------------------------------------------------------------------------------------------
def project(cams: CameraSet, pts: torch.Tensor, want_ndc=True, want_yx=True):
    frames, P = pts.shape[0], pts.shape[1]
    N = frames * cams.views
    ndc = torch.empty(N, P, 3, dtype=torch.float32, device=pts.device) if want_ndc else None
    yx = torch.empty(N, P, 2, dtype=torch.float32, device=pts.device) if want_yx else None
    c = cams.struct(N)
    _lib.checked().smil_project(ctypes.byref(c), _ptr(pts), P, _ptr(ndc), _ptr(yx), _stream())
    return ndc, yx


def project_backward(cams: CameraSet, pts: torch.Tensor, d_ndc=None, d_yx=None, d_pts=None, d_fov_img=None,
                     accumulate=False, d_ndc_scale=None):
    frames, P = pts.shape[0], pts.shape[1]
    N = frames * cams.views
    if d_pts is None:
        d_pts = torch.empty_like(pts)
        accumulate = False
    if d_fov_img is None:
        d_fov_img = torch.zeros(N, dtype=torch.float32, device=pts.device)
    c = cams.struct(N)
    _lib.checked().smil_project_backward(ctypes.byref(c), _ptr(pts), P, _ptr(d_ndc), _ptr(d_yx), _ptr(d_pts), _ptr(d_fov_img), int(accumulate),
                                         _ptr(d_ndc_scale), _stream())
    return d_pts, d_fov_img


def project_verts_and_joints(cams: CameraSet, verts: torch.Tensor, joints: torch.Tensor):
    """One launch: verts (frames,V,3) -> NDC (N,V,3) for the rasteriser, joints (frames,J,3) -> (y,x) pixels (N,J,2)."""
    frames, V, J = verts.shape[0], verts.shape[1], joints.shape[1]
    N = frames * cams.views
    ndc = torch.empty(N, V, 3, dtype=torch.float32, device=verts.device)
    yx = torch.empty(N, J, 2, dtype=torch.float32, device=verts.device)
    c = cams.struct(N)
    _lib.checked().smil_project2(ctypes.byref(c), _ptr(verts), V, _ptr(ndc), None, _ptr(joints), J, None, _ptr(yx), _stream())
    return ndc, yx


def project_backward_verts_and_joints(cams: CameraSet, verts, d_ndc, joints, d_yx, d_fov_img, d_ndc_scale=None):
    """One launch: the backward of ``project_verts_and_joints``; returns (d_verts, d_joints), adds to d_fov_img.
    ``d_ndc_scale``: the decode factors of a ``d_ndc`` the fused rasteriser left packed (``silhouette_l1_fused(packed_out=True)``)."""
    V, J = verts.shape[1], joints.shape[1]
    N = verts.shape[0] * cams.views
    d_verts, d_joints = torch.empty_like(verts), torch.empty_like(joints)
    c = cams.struct(N)
    _lib.checked().smil_project_backward2(ctypes.byref(c), _ptr(verts), V, _ptr(d_ndc), None, _ptr(d_verts), _ptr(joints), J, None, _ptr(d_yx),
                                          _ptr(d_joints), _ptr(d_fov_img), _ptr(d_ndc_scale), _stream())
    return d_verts, d_joints


def fit_epilogue(cfg, pose, trans, betas, mean_betas, betas_prec, mask, objs, d_pose, d_trans, d_betas, halo_prev=None, halo_next=None,
                 accumulate=True, loss_img=None, pix_scale=None, cams: Optional[CameraSet] = None, d_fov_img=None, d_fov=None):
    """prior_losses + sil_objective + fov_reduce in one launch (the tail of a fit iteration)."""
    n_img = 0 if loss_img is None else loss_img.numel()
    c = None if cams is None else cams.struct(d_fov_img.numel())
    _lib.checked().smil_fit_epilogue(ctypes.byref(cfg), _ptr(pose), _ptr(trans), _ptr(betas), _ptr(mean_betas), _ptr(betas_prec), _ptr(mask),
                                     _ptr(halo_prev), _ptr(halo_next), _ptr(objs), _ptr(d_pose), _ptr(d_trans), _ptr(d_betas), int(accumulate),
                                     _ptr(loss_img), _ptr(pix_scale), n_img, None if c is None else ctypes.byref(c), _ptr(d_fov_img), _ptr(d_fov),
                                     _stream())


def fov_reduce(cams: CameraSet, d_fov_img: torch.Tensor) -> torch.Tensor:
    N = d_fov_img.numel()
    d_fov = torch.empty(cams.fov.numel(), dtype=torch.float32, device=d_fov_img.device)
    c = cams.struct(N)
    _lib.checked().smil_fov_reduce(ctypes.byref(c), _ptr(d_fov_img), _ptr(d_fov), _stream())
    return d_fov


# ----------------------------------------------------------------------------------------------
# silhouette
# ----------------------------------------------------------------------------------------------
# The per-image tables of one rasteriser launch (tile boxes, depth ranges, work lists: ~12 F + 8 tiles bytes per image) are
# part of the workspace; launches are cut into slices of this many images so that the workspace stays bounded at cfg5
# scale (147 k images per GPU).  Each slice still holds millions of tiles.
MAX_IMAGES_PER_LAUNCH = 16384
MAX_WORKSPACE_BYTES = 24 << 30  # the per-image tables (incl. the binned tile lists, ~96-192 bytes per face) shrink the slice until this holds


def _slice_images(model: "DeviceModel", N: int, S: int) -> int:
    """Images per rasteriser call: at most MAX_IMAGES_PER_LAUNCH, fewer when the per-image workspace tables would push the
    workspace past MAX_WORKSPACE_BYTES (mouse-sized meshes at 512^2)."""
    step = min(N, MAX_IMAGES_PER_LAUNCH)
    key = (N, S, step)
    cached = model.__dict__.setdefault("_slice_cache", {})
    if key not in cached:
        while step > 256 and int(_lib.load().smil_raster_workspace_bytes(model.handle, step, S)) > MAX_WORKSPACE_BYTES:
            step = (step + 1) // 2
        cached[key] = step
    return cached[key]


def _slices(N: int, step: int = MAX_IMAGES_PER_LAUNCH):
    for n0 in range(0, N, step):
        yield n0, min(N, n0 + step)


def raster_stats(model: DeviceModel, N: int) -> dict:
    """Counters of the most recent rasteriser call of ``model`` (of its last slice when the batch was cut into several launches):
    faces straddling z_clip, touched tiles, faces beyond the clip tables, pixels replayed through the reference's queue (``tie_rule``).  ``N`` is ignored (kept for callers of round 3): the
    counters lie at the start of the workspace whatever the slice size.  Zeros when the model has not rasterised since the workspace was
    last used by another model.  Synchronises."""
    zero = {"straddling_faces": 0, "tiles": 0, "unclipped_faces": 0, "tie_pixels": 0}
    user = _WS_USER.get(model._ws_key())
    if model._ws is None or user is None or user[0] is not model:
        return zero  # this model has not rasterised, or another model / topology has used the shared workspace since
    out = (ctypes.c_uint32 * 4)()
    _lib.checked().smil_raster_stats(model.handle, _ptr(model._ws), _stream(), out)
    return {"straddling_faces": int(out[0]), "tiles": int(out[1]), "unclipped_faces": int(out[2]), "tie_pixels": int(out[3])}


def silhouette_forward(model: DeviceModel, verts_ndc: torch.Tensor, S: int, rs=None) -> torch.Tensor:
    rs = rs or raster_settings()
    N = verts_ndc.shape[0]
    sil = torch.empty(N, S, S, dtype=torch.float32, device=verts_ndc.device)
    step = model._last_slice = _slice_images(model, N, S)
    ws = model.workspace(step, S)
    model._claim_workspace()
    for n0, n1 in _slices(N, step):
        _lib.checked().smil_silhouette_forward(model.handle, _ptr(verts_ndc[n0:n1]), n1 - n0, S, ctypes.byref(rs), _ptr(sil[n0:n1]), _ptr(ws),
                                               _stream())
    return sil


def silhouette_backward(model: DeviceModel, verts_ndc: torch.Tensor, S: int, grad_sil: torch.Tensor, rs=None,
                        clip_depth: Optional[ClipDepth] = None) -> torch.Tensor:
    """``clip_depth``: receives the depth gradients of the end points of edges that cross the clipping plane (``ClipDepth``)."""
    rs = rs or raster_settings()
    N = verts_ndc.shape[0]
    d_ndc = torch.empty(N, model.V, 2, dtype=torch.float32, device=verts_ndc.device)
    step = model._last_slice = _slice_images(model, N, S)
    ws = model.workspace(step, S)
    model._claim_workspace()
    for n0, n1 in _slices(N, step):
        _lib.checked().smil_silhouette_backward(model.handle, _ptr(verts_ndc[n0:n1]), n1 - n0, S, ctypes.byref(_rs_for_slice(rs, clip_depth, n0)),
                                                _ptr(grad_sil[n0:n1]), _ptr(d_ndc[n0:n1]), _ptr(ws), _stream())
    return d_ndc


def silhouette_l1_fused(model: DeviceModel, verts_ndc, S, target, target_sum, pix_scale, rs=None, want_sil=False,
                        loss_img=None, d_ndc=None, packed_out=False, clip_depth: Optional[ClipDepth] = None):
    """Fused soft silhouette + L1 + backward.  Returns (loss_img, d_ndc, sil), or with ``packed_out`` (loss_img, d_ndc, sil,
    d_ndc_scale): ``d_ndc`` as the kernel accumulated it (64-bit packed fixed point for large batches) plus the per-image
    decode factors ``project_backward`` takes - this saves the decode pass over the whole gradient."""
    rs = rs or raster_settings()
    N = verts_ndc.shape[0]
    dev = verts_ndc.device
    if loss_img is None:
        loss_img = torch.empty(N, dtype=torch.float32, device=dev)
    if d_ndc is None:
        d_ndc = torch.empty(N, model.V, 2, dtype=torch.float32, device=dev)
    sil = torch.empty(N, S, S, dtype=torch.float32, device=dev) if want_sil else None
    scale = torch.empty(N, dtype=torch.float32, device=dev) if packed_out else None
    step = model._last_slice = _slice_images(model, N, S)
    ws = model.workspace(step, S)
    model._claim_workspace()
    if target.dtype not in (torch.float32, torch.uint8):
        raise _lib.SmilError(f"target silhouettes must be float32 or uint8, got {target.dtype}")
    for n0, n1 in _slices(N, step):
        _lib.checked().smil_silhouette_l1_fused(model.handle, _ptr(verts_ndc[n0:n1]), n1 - n0, S, ctypes.byref(_rs_for_slice(rs, clip_depth, n0)),
                                                _ptr(target[n0:n1]), int(target.dtype == torch.uint8), _ptr(target_sum[n0:n1]),
                                                _ptr(pix_scale[n0:n1]), _ptr(loss_img[n0:n1]), _ptr(d_ndc[n0:n1]),
                                                _ptr(None if sil is None else sil[n0:n1]), _ptr(None if scale is None else scale[n0:n1]), _ptr(ws),
                                                _stream())
    return (loss_img, d_ndc, sil, scale) if packed_out else (loss_img, d_ndc, sil)


# ----------------------------------------------------------------------------------------------
# colour (HardPhong)
# ----------------------------------------------------------------------------------------------
_COLOUR_WS: Dict = {}  # (device type, index) -> the device's colour workspace (tables only: no per-workgroup streams)
MAX_COLOUR_WORKSPACE_BYTES = 8 << 30  # frames per colour launch shrink until the workspace fits this


def _colour_workspace(model: DeviceModel, N: int, S: int, size_of=None) -> torch.Tensor:
    need = int((size_of or _lib.load().smil_colour_workspace_bytes)(model.handle, N, S))
    key = model._ws_key()
    ws = _COLOUR_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _COLOUR_WS[key] = _workspace(need, model.device)
    return ws


def render_colour(model: DeviceModel, cams: CameraSet, verts: torch.Tensor, mesh_color, verts_ndc: Optional[torch.Tensor] = None,
                  want_pix_to_face: bool = False):
    """HardPhong colour image of the reference Renderer's colour branch (p3d_renderer.py:54-70,148-150): ``verts`` (frames,V,3) world
    space, ``mesh_color`` three floats in [0, 1] -> (N,3,S,S) float32 with N = frames * views (background 1.0), and with
    ``want_pix_to_face`` also the (N,S,S) int32 original face id per pixel (-1: background).  ``verts_ndc``: the projection of ``verts``
    through ``cams`` when the caller has it.  No gradient (visualisation only).  Large batches are cut into launches of whole frames."""
    verts = verts.detach().float().contiguous()
    frames, V = verts.shape[0], verts.shape[1]
    views, S = cams.views, cams.S
    N = frames * views
    dev = verts.device
    if verts_ndc is None:
        verts_ndc, _ = project(cams, verts, want_yx=False)
    verts_ndc = verts_ndc.detach().float().contiguous()
    image = torch.empty(N, 3, S, S, dtype=torch.float32, device=dev)
    p2f = torch.empty(N, S, S, dtype=torch.int32, device=dev) if want_pix_to_face else None
    rgb = (ctypes.c_float * 3)(*[float(c) for c in mesh_color])
    lib = _lib.checked()
    step = frames  # frames per launch
    while step > 1 and int(lib.smil_colour_workspace_bytes(model.handle, step * views, S)) > MAX_COLOUR_WORKSPACE_BYTES:
        step = (step + 1) // 2
    ws = _colour_workspace(model, step * views, S)
    for f0 in range(0, frames, step):
        f1 = min(frames, f0 + step)
        n0, n1 = f0 * views, f1 * views

        def rows(t):  # camera tables with one row per image follow the slice; shared / per-view ones stay
            return t if t is None or t.shape[0] != N or n1 - n0 == N else t[n0:n1].contiguous()
        part = CameraSet(rows(cams.R), rows(cams.T), rows(cams.fov.reshape(-1)), rows(None if cams.aspect is None else cams.aspect.reshape(-1)),
                         views, S, rows(cams.principal))
        c = part.struct(n1 - n0)
        lib.smil_render_colour(model.handle, ctypes.byref(c), _ptr(verts[f0:f1]), _ptr(verts_ndc[n0:n1]), rgb, _ptr(image[n0:n1]),
                               _ptr(None if p2f is None else p2f[n0:n1]), _ptr(ws), _stream())
    return (image, p2f) if want_pix_to_face else image


class Fragments(NamedTuple):
    """What ``render_fragments`` returns; an output that was not asked for is None.  Unlike pytorch3d's ``Fragments`` there is no K axis
    (K = 1), face ids count within the image's own mesh (int32, not packed over the batch) and there is no ``dists`` (blur 0)."""

    pix_to_face: Optional[torch.Tensor]  # (N,S,S) int32, -1: background
    zbuf: Optional[torch.Tensor]         # (N,S,S) float32 view depth, -1: background
    bary: Optional[torch.Tensor]         # (N,S,S,3) float32 with respect to the original face, -1: background
    dist: Optional[torch.Tensor]         # (N,S,S) float32 distance camera centre -> surface, +inf: background


FRAGMENT_OUTPUTS = Fragments._fields


def _camera_rows(cams: CameraSet, N: int, n0: int, n1: int) -> CameraSet:
    """The cameras of images [n0, n1) of N: tables with one row per image follow the slice; shared / per-view ones stay."""
    def rows(t):
        return t if t is None or t.shape[0] != N or n1 - n0 == N else t[n0:n1].contiguous()
    return CameraSet(rows(cams.R), rows(cams.T), rows(cams.fov.reshape(-1)), rows(None if cams.aspect is None else cams.aspect.reshape(-1)),
                     cams.views, cams.S, rows(cams.principal))


def render_fragments(model: DeviceModel, cams: CameraSet, verts: torch.Tensor, verts_ndc: Optional[torch.Tensor] = None,
                     want=FRAGMENT_OUTPUTS) -> Fragments:
    """The hard rasteriser's result (blur 0, K = 1: the rasterisation of ``render_colour``, p3d_renderer.py:54-70) for ``verts``
    (frames,V,3) in world space: the outputs named in ``want`` as a ``Fragments`` tuple over N = frames * views images.  ``dist`` is the
    depth pass's convention, the Euclidean distance from the camera centre to the surface point.  ``verts_ndc``: the projection of
    ``verts`` through ``cams`` when the caller has it.  No gradient.  Large batches are cut into launches of whole frames of at most
    ``MAX_IMAGES_PER_LAUNCH`` images."""
    want = tuple(want)
    unknown = [w for w in want if w not in FRAGMENT_OUTPUTS]
    if unknown or not want:
        raise ValueError(f"want must name some of {FRAGMENT_OUTPUTS}, got {want}")
    verts = verts.detach().float().contiguous()
    frames, V = verts.shape[0], verts.shape[1]
    views, S = cams.views, cams.S
    N = frames * views
    dev = verts.device
    if verts_ndc is None:
        verts_ndc, _ = project(cams, verts, want_yx=False)
    verts_ndc = verts_ndc.detach().float().contiguous()
    shapes = dict(pix_to_face=((N, S, S), torch.int32), zbuf=((N, S, S), torch.float32), bary=((N, S, S, 3), torch.float32),
                  dist=((N, S, S), torch.float32))
    out = {k: (torch.empty(*shapes[k][0], dtype=shapes[k][1], device=dev) if k in want else None) for k in FRAGMENT_OUTPUTS}
    lib = _lib.checked()
    step = max(1, min(frames, MAX_IMAGES_PER_LAUNCH // views))  # frames per launch
    while step > 1 and int(lib.smil_fragments_workspace_bytes(model.handle, step * views, S)) > MAX_COLOUR_WORKSPACE_BYTES:
        step = (step + 1) // 2
    ws = _colour_workspace(model, step * views, S, lib.smil_fragments_workspace_bytes)
    for f0 in range(0, frames, step):
        f1 = min(frames, f0 + step)
        n0, n1 = f0 * views, f1 * views
        c = _camera_rows(cams, N, n0, n1).struct(n1 - n0)
        part = [_ptr(None if out[k] is None else out[k][n0:n1]) for k in FRAGMENT_OUTPUTS]
        lib.smil_render_fragments(model.handle, ctypes.byref(c), _ptr(verts[f0:f1]), _ptr(verts_ndc[n0:n1]), *part, _ptr(ws), _stream())
    return Fragments(**out)


def depth_visibility(depth: torch.Tensor, kp_norm: torch.Tensor, kp_dist: torch.Tensor, visibility: torch.Tensor, tolerance: float,
                     neighborhood: int = 1, depth_max: Optional[float] = None, want_surface: bool = False):
    """Keypoint self-occlusion against a depth buffer (Unreal2Pytorch3D.py:733-758 for B images at once, float64 comparisons).
    ``depth``: uint8 (B,H,W,C) with the depth in channel 0 and ``depth_max`` (surface = r / 255 * depth_max), or float32 (B,H,W)
    distances with +inf as background.  ``kp_norm`` (B,P,2) float64 = (row / H, column / W), the reference's swapped convention;
    ``kp_dist`` (B,P) float64 distance of every keypoint to its camera (non-finite: no 3-D position); ``visibility`` (B,P) float32.
    Returns the refined (B,P) float32 visibility (it only ever turns non-zero into 0), with ``want_surface`` also the (B,P) float64
    sampled surface distance (NaN where none was sampled).  ``neighborhood``: half-window in pixels, 0 to 8."""
    dev = require_gpu(depth.device)
    if depth.dtype == torch.uint8:
        if depth.dim() != 4 or depth.shape[3] < 1:
            raise _lib.SmilError(f"a uint8 depth buffer must be (B,H,W,C), got {tuple(depth.shape)}")
        if depth_max is None:
            raise _lib.SmilError("a uint8 depth buffer needs depth_max")
        channels = int(depth.shape[3])
    elif depth.dtype == torch.float32:
        if depth.dim() != 3:
            raise _lib.SmilError(f"a float32 depth buffer must be (B,H,W), got {tuple(depth.shape)}")
        channels = 1
    else:
        raise _lib.SmilError(f"the depth buffer must be uint8 or float32, got {depth.dtype}")
    B, H, W = int(depth.shape[0]), int(depth.shape[1]), int(depth.shape[2])
    if kp_norm.dim() != 3 or kp_norm.shape[0] != B or kp_norm.shape[2] != 2:
        raise _lib.SmilError(f"kp_norm must be ({B},P,2), got {tuple(kp_norm.shape)}")
    P = int(kp_norm.shape[1])
    for name, t, dt in (("kp_norm", kp_norm, torch.float64), ("kp_dist", kp_dist, torch.float64), ("visibility", visibility, torch.float32)):
        if t.dtype != dt or t.device != dev:
            raise _lib.SmilError(f"{name} must be {dt} on {dev}, got {t.dtype} on {t.device}")
    if tuple(kp_dist.shape) != (B, P) or tuple(visibility.shape) != (B, P):
        raise _lib.SmilError(f"kp_dist and visibility must be ({B},{P}), got {tuple(kp_dist.shape)} and {tuple(visibility.shape)}")
    depth, kp_norm, kp_dist, visibility = depth.contiguous(), kp_norm.contiguous(), kp_dist.contiguous(), visibility.contiguous()
    out = torch.empty(B, P, dtype=torch.float32, device=dev)
    surface = torch.empty(B, P, dtype=torch.float64, device=dev) if want_surface else None
    _lib.checked().smil_depth_visibility(_ptr(depth), int(depth.dtype == torch.uint8), channels, float(0.0 if depth_max is None else depth_max), B, H,
                                         W, _ptr(kp_norm), _ptr(kp_dist), P, _ptr(visibility), float(tolerance), int(neighborhood), _ptr(out),
                                         _ptr(surface), _stream())
    return (out, surface) if want_surface else out


def image_abs_sum(images: torch.Tensor) -> torch.Tensor:
    N = images.shape[0]
    pixels = images[0].numel()
    out = torch.empty(N, dtype=torch.float32, device=images.device)
    _lib.checked().smil_image_abs_sum(_ptr(images), int(images.dtype == torch.uint8), N, pixels, _ptr(out), _stream())
    return out


# ----------------------------------------------------------------------------------------------
# losses / optimiser
# ----------------------------------------------------------------------------------------------
def fit_config(N, J, nB, window, weights, w_temp=0.0, frame0=0, N_total=None, limit=0.01, train_global=True,
               train_joints=True, train_trans=True) -> _lib.FitConfig:
    """weights in the reference order (fitter.py:238): w_j2d, w_reproj, w_betas, w_pose, w_limit, w_splay."""
    c = _lib.FitConfig()
    c.train_global, c.train_joints, c.train_trans = int(train_global), int(train_joints), int(train_trans)
    c.N, c.J, c.nB, c.window, c.frame0 = N, J, nB, window, frame0
    c.N_total = N if N_total is None else N_total
    c.w_j2d, c.w_reproj, c.w_betas, c.w_pose, c.w_limit, c.w_splay = [float(w) for w in weights]
    c.w_temp, c.limit = float(w_temp), float(limit)
    return c


def pix_scale(cfg: _lib.FitConfig, views: int, S: int, device) -> torch.Tensor:
    out = torch.empty(cfg.N * views, dtype=torch.float32, device=device)
    _lib.checked().smil_pix_scale(ctypes.byref(cfg), views, S, _ptr(out), _stream())
    return out


def prior_losses(cfg, pose, trans, betas, mean_betas, betas_prec, mask, objs, d_pose, d_trans, d_betas, halo_prev=None,
                 halo_next=None, accumulate=True):
    """pose (N,J,3) = [global_rotation ; joint_rotations], mask (J,3) = [global_mask ; rotation_mask]."""
    _lib.checked().smil_prior_losses(ctypes.byref(cfg), _ptr(pose), _ptr(trans), _ptr(betas), _ptr(mean_betas), _ptr(betas_prec), _ptr(mask),
                                     _ptr(halo_prev), _ptr(halo_next), _ptr(objs), _ptr(d_pose), _ptr(d_trans), _ptr(d_betas), int(accumulate),
                                     _stream())


def mask_rows(x: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    cols = mask.numel()
    out = torch.empty_like(x) if out is None else out
    _lib.checked().smil_mask_rows(_ptr(x), _ptr(mask), x.numel() // cols, cols, _ptr(out), _stream())
    return out


def joint_loss(cfg, views, Jc, canon, proj, target, visibility, objs, d_proj):
    _lib.checked().smil_joint_loss(ctypes.byref(cfg), views, Jc, _ptr(canon), _ptr(proj), _ptr(target), _ptr(visibility), _ptr(objs), _ptr(d_proj),
                                   _stream())


def sil_objective(loss_img, pscale, objs):
    _lib.checked().smil_sil_objective(_ptr(loss_img), _ptr(pscale), loss_img.numel(), _ptr(objs), _stream())


def window_terms(cfg, views, Jc, canon, proj, target, visibility, pose, mask, objs_total, loss_img, pscale) -> torch.Tensor:
    """(windows of this shard, 6) = [joint, limit, pose, splay, betas, sil_reproj] of every window, from the buffers of ONE
    whole-batch iteration (``smil_window_terms``): what the reference's per-window ``forward`` calls of an epoch return."""
    w = cfg.window if cfg.window > 0 else cfg.N_total
    n_win = (cfg.N + w - 1) // w
    out = torch.empty(n_win, 6, dtype=torch.float32, device=pose.device)
    _lib.checked().smil_window_terms(ctypes.byref(cfg), views, Jc, _ptr(canon), _ptr(proj), _ptr(target), _ptr(visibility), _ptr(pose), _ptr(mask),
                                     _ptr(objs_total), _ptr(loss_img), _ptr(pscale), _ptr(out), n_win, _stream())
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.5, beta2=0.999, eps=1e-8):
    _lib.checked().smil_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), lr, beta1, beta2, eps, step, _stream())


def _adam_multi(entry, items, beta1, beta2, eps):
    """``items`` packed as SmilAdamTensor arrays, ADAM_MAX_TENSORS to a launch of the library's ``entry``."""
    for k0 in range(0, len(items), _lib.ADAM_MAX_TENSORS):
        chunk = items[k0:k0 + _lib.ADAM_MAX_TENSORS]
        arr = (_lib.AdamTensor * len(chunk))()
        for a, (p, g, m, v, lr, step) in zip(arr, chunk):
            a.param, a.grad, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            a.n, a.lr, a.step = p.numel(), float(lr), int(step)
        getattr(_lib.checked(), entry)(arr, len(chunk), beta1, beta2, eps, _stream())


def adam_step_multi(items, beta1=0.5, beta2=0.999, eps=1e-8):
    """One launch for several tensors: ``items`` = [(param, grad, exp_avg, exp_avg_sq, lr, step), ...]."""
    _adam_multi("smil_adam_step_multi", items, beta1, beta2, eps)


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, lr, step_dev, step_offset=0, beta1=0.5, beta2=0.999, eps=1e-8):
    """Adam update whose step count is ``step_dev[0] - step_offset`` (int32 device tensor): capturable in a hipGraph."""
    _lib.checked().smil_adam_step_dev(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), lr, beta1, beta2, eps, _ptr(step_dev),
                                      int(step_offset), _stream())


def profile_enable(on: bool) -> None:
    _lib.checked().smil_profile_enable(int(on))


def profile_read():
    """(summed tile-kernel milliseconds, launches) since the last enable/read."""
    ms, n = ctypes.c_float(), ctypes.c_int32()
    _lib.checked().smil_profile_read(ctypes.byref(ms), ctypes.byref(n))
    return float(ms.value), int(n.value)


# ---- 3-D scan registration losses (mesh3d.hip) ------------------------------------------------------------------------------
def sample_points(verts_packed: torch.Tensor, faces_packed: torch.Tensor, face_off: torch.Tensor, cum_area: torch.Tensor, n_meshes: int,
                  num_samples: int, seed: int, want_faces: bool = False):
    """(N, S, 3) surface samples of N packed meshes; faces_packed (F,3) int32 into the packed verts, face_off (N+1) int32,
    cum_area (F) float64 per-mesh normalised cumulative areas.  With want_faces also the (N, S) face index within each mesh."""
    dev = verts_packed.device
    out = torch.empty(n_meshes, num_samples, 3, device=dev, dtype=torch.float32)
    fidx = torch.empty(n_meshes, num_samples, device=dev, dtype=torch.int32) if want_faces else None
    _lib.checked().smil_sample_points(_ptr(verts_packed), int(verts_packed.shape[0]), _ptr(faces_packed), _ptr(face_off), _ptr(cum_area),
                                      int(n_meshes), int(num_samples), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _ptr(fidx), _stream())
    return out, fidx


def chamfer(x: torch.Tensor, y: torch.Tensor, single_directional=False, point_sum=False, batch_sum=False, want_grad=True):
    """Chamfer loss of x (N,P1,3) and y (N,P2,3): (loss (1,), idx_x (N,P1), idx_y (N,P2) or None, d_x, d_y or None)."""
    N, P1, P2 = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    dev = x.device
    lib = _lib.checked()
    ws = _workspace(lib.smil_chamfer_workspace_bytes(N, P1, P2), dev)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    idx_x = torch.empty(N, P1, device=dev, dtype=torch.int32)
    idx_y = None if single_directional else torch.empty(N, P2, device=dev, dtype=torch.int32)
    d_x = torch.empty_like(x) if want_grad else None
    d_y = torch.empty_like(y) if want_grad else None
    lib.smil_chamfer(_ptr(x), _ptr(y), N, P1, P2, int(bool(single_directional)), int(bool(point_sum)), int(bool(batch_sum)), _ptr(loss), _ptr(idx_x),
                     _ptr(idx_y), _ptr(d_x), _ptr(d_y), _ptr(ws), _stream())
    return loss, idx_x, idx_y, d_x, d_y


def _check_knn_sizes(what: str, P1: int, P2: int, K: int, both: bool, min_points: int = 1) -> None:
    if not 1 <= K <= _lib.KNN_MAX_K:
        raise ValueError(f"{what}: K={K} outside 1 .. {_lib.KNN_MAX_K} (SMIL_KNN_MAX_K)")
    if K > P2 or (both and K > P1):
        raise ValueError(f"{what}: K={K} exceeds the number of candidate points (P1={P1}, P2={P2})")
    if min(P1, P2) < min_points:
        raise ValueError(f"{what}: every cloud needs at least {min_points} points (P1={P1}, P2={P2})")


def _insertions(ws: torch.Tensor) -> torch.Tensor:
    return ws[:8].view(torch.int64)


def knn(x: torch.Tensor, y: torch.Tensor, K: int, both: bool = False):
    """The K nearest points of y (N,P2,3) for every point of x (N,P1,3), ascending by (squared distance, index):
    (dists_x (N,P1,K), idx_x (N,P1,K) int32, dists_y, idx_y (N,P2,K) or None, insertions (1,) int64 on the device)."""
    N, P1, P2, K = int(x.shape[0]), int(x.shape[1]), int(y.shape[1]), int(K)
    _check_knn_sizes("knn", P1, P2, K, both)
    dev = x.device
    lib = _lib.checked()
    ws = _workspace(lib.smil_knn_workspace_bytes(N, P1, P2, K), dev)
    dx = torch.empty(N, P1, K, device=dev, dtype=torch.float32)
    ix = torch.empty(N, P1, K, device=dev, dtype=torch.int32)
    dy = torch.empty(N, P2, K, device=dev, dtype=torch.float32) if both else None
    iy = torch.empty(N, P2, K, device=dev, dtype=torch.int32) if both else None
    lib.smil_knn(_ptr(x), _ptr(y), N, P1, P2, K, _ptr(dx), _ptr(ix), _ptr(dy), _ptr(iy), _ptr(ws), _stream())
    return dx, ix, dy, iy, _insertions(ws)


def sdf_distance(x: torch.Tensor, y: torch.Tensor, x_sdf: torch.Tensor, y_sdf: torch.Tensor, K: int, single_directional=False,
                 point_sum=False, batch_sum=False, want_grad=True, want_tables=False):
    """The SDF-guided term of x (N,P1,3), y (N,P2,3) with per-point values x_sdf (N,P1), y_sdf (N,P2): (loss (1,), d_x, d_y or
    None, tables (dists_x, idx_x, dists_y, idx_y) or None, insertions (1,) int64 on the device)."""
    N, P1, P2, K = int(x.shape[0]), int(x.shape[1]), int(y.shape[1]), int(K)
    _check_knn_sizes("sdf_distance", P1, P2, K, not single_directional, min_points=2)
    dev = x.device
    lib = _lib.checked()
    ws = _workspace(lib.smil_sdf_distance_workspace_bytes(N, P1, P2, K), dev)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    d_x = torch.empty_like(x) if want_grad else None
    d_y = torch.empty_like(y) if want_grad else None
    tables = None
    if want_tables:
        tables = (torch.empty(N, P1, K, device=dev, dtype=torch.float32), torch.empty(N, P1, K, device=dev, dtype=torch.int32),
                  None if single_directional else torch.empty(N, P2, K, device=dev, dtype=torch.float32),
                  None if single_directional else torch.empty(N, P2, K, device=dev, dtype=torch.int32))
    t = tables or (None,) * 4
    lib.smil_sdf_distance(_ptr(x), _ptr(y), _ptr(x_sdf), _ptr(y_sdf), N, P1, P2, K, int(bool(single_directional)), int(bool(point_sum)),
                          int(bool(batch_sum)), _ptr(loss), _ptr(d_x), _ptr(d_y), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _ptr(ws), _stream())
    return loss, d_x, d_y, tables, _insertions(ws)


def sample_vertices(verts_packed: torch.Tensor, values_packed: torch.Tensor, vert_off: torch.Tensor, n_meshes: int, num_samples: int,
                    seed: int):
    """(points (N,S,3), values (N,S), vertex index within its mesh (N,S) int32) of S vertices drawn uniformly with replacement from each
    of N packed meshes; vert_off (N+1) int32."""
    dev = verts_packed.device
    out = torch.empty(n_meshes, num_samples, 3, device=dev, dtype=torch.float32)
    val = torch.empty(n_meshes, num_samples, device=dev, dtype=torch.float32)
    idx = torch.empty(n_meshes, num_samples, device=dev, dtype=torch.int32)
    _lib.checked().smil_sample_vertices(_ptr(verts_packed), _ptr(values_packed), _ptr(vert_off), int(n_meshes), int(num_samples),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _ptr(val), _ptr(idx), _stream())
    return out, val, idx


def sample_vertices_backward(d_pts: torch.Tensor, idx: torch.Tensor, vert_off: torch.Tensor, n_verts: int, max_verts: int):
    """d_verts (n_verts,3): d_pts (N,S,3) summed over the samples that drew each vertex (order-independent)."""
    N, S = int(idx.shape[0]), int(idx.shape[1])
    lib = _lib.checked()
    ws = _workspace(lib.smil_sample_vertices_backward_workspace_bytes(int(n_verts), N), d_pts.device)
    d_verts = torch.empty(int(n_verts), 3, device=d_pts.device, dtype=torch.float32)
    lib.smil_sample_vertices_backward(_ptr(d_pts), _ptr(idx), _ptr(vert_off), int(n_verts), int(max_verts), N, S, _ptr(d_verts), _ptr(ws), _stream())
    return d_verts


class DeviceTopology:
    """The regulariser tables of one face array (``mesh3d.Topology``) resident on one GPU (``SmilMeshTopology``)."""

    def __init__(self, topo, device):
        self.device = require_gpu(device)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1)).to(self.device)  # noqa: E731
        self.tensors = dict(edges=i32(topo.edges), pairs=i32(topo.pairs), nbr_ptr=i32(topo.nbr_ptr), nbr=i32(topo.nbr),
                            inv_deg=torch.from_numpy(np.ascontiguousarray(topo.inv_deg, np.float32)).to(self.device),
                            vpair_ptr=i32(topo.vpair_ptr), vpair=i32(topo.vpair))
        s = _lib.MeshTopology()
        s.V, s.E, s.Q = int(topo.V), int(topo.E), int(topo.Q)
        for k, t in self.tensors.items():
            setattr(s, k, t.data_ptr() if t.numel() else None)
        self.struct = s
        self.V = topo.V


def mesh_regularisers(topo: DeviceTopology, verts: torch.Tensor, terms: int, want_grad=True):
    """verts (B,V,3) on ``topo`` -> (out3 (3,) = edge, normal, laplacian losses, d_edge, d_normal, d_lap (B,V,3) or None)."""
    B = int(verts.shape[0])
    lib = _lib.checked()
    ws = _workspace(lib.smil_mesh_reg_workspace_bytes(ctypes.byref(topo.struct), B), verts.device)
    out = torch.empty(3, device=verts.device, dtype=torch.float32)
    g = [torch.empty_like(verts) if (want_grad and terms & bit) else None for bit in (_lib.REG_EDGE, _lib.REG_NORMAL, _lib.REG_LAPLACIAN)]
    lib.smil_mesh_regularisers(ctypes.byref(topo.struct), _ptr(verts), B, int(terms), _ptr(out), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(ws),
                               _stream())
    return out, g[0], g[1], g[2]


# ---- spatial-diameter values by ray casting (raycast.hip) -------------------------------------------------------------------------
def ray_diameters(verts: torch.Tensor, faces: torch.Tensor, origins: torch.Tensor, own_face: torch.Tensor, dirs: torch.Tensor, t_min: float,
                  d_lo: float, d_hi: float, cap: int, want_ray_t: bool = False):
    """S samples with R rays each against every face of one mesh: verts (V,3) float32, faces (F,3) int32, origins (S,3), own_face (S)
    int32, dirs (S,R,3).  (diam (S), ray_t (S,R) or None): a ray's value is the largest t over its hits (-1: none), a sample's the
    mean of its first ``cap`` rays with d_lo < t < d_hi in ray order, or d_lo (smil_ray_diameters, include/smilfit.h)."""
    V, F, S, R = int(verts.shape[0]), int(faces.shape[0]), int(dirs.shape[0]), int(dirs.shape[1])
    if verts.dtype != torch.float32 or origins.dtype != torch.float32 or dirs.dtype != torch.float32:
        raise ValueError("ray_diameters: verts, origins and dirs must be float32")
    if faces.dtype != torch.int32 or own_face.dtype != torch.int32:
        raise ValueError("ray_diameters: faces and own_face must be int32")
    if tuple(verts.shape) != (V, 3) or tuple(faces.shape) != (F, 3) or tuple(origins.shape) != (S, 3) or tuple(own_face.shape) != (S,) \
            or tuple(dirs.shape) != (S, R, 3):
        raise ValueError("ray_diameters: verts (V,3), faces (F,3), origins (S,3), own_face (S), dirs (S,R,3)")
    dev = verts.device
    verts, faces, origins, own_face, dirs = (t.contiguous() for t in (verts, faces, origins, own_face, dirs))
    lib = _lib.checked()
    ws = _workspace(lib.smil_ray_diameters_workspace_bytes(F, S, R), dev)
    diam = torch.empty(S, device=dev, dtype=torch.float32)
    ray_t = torch.empty(S, R, device=dev, dtype=torch.float32) if want_ray_t else None
    lib.smil_ray_diameters(_ptr(verts), V, _ptr(faces), F, _ptr(origins), _ptr(own_face), _ptr(dirs), S, R, float(t_min), float(d_lo), float(d_hi),
                           int(cap), _ptr(ray_t), _ptr(diam), _ptr(ws), _stream())
    return diam, ray_t


# ---- exact point <-> triangle-mesh distances (point_mesh.hip) --------------------------------------------------------------------
class MeshTables(NamedTuple):
    """N packed meshes as the point-mesh kernels take them (``mesh3d.Meshes.face_tables``): faces (F_total,3) int32 into the packed
    vertices, face_off / vert_off (N+1) int32 on the device, and the sizes the launches need on the host."""
    faces: torch.Tensor
    face_off: torch.Tensor
    vert_off: torch.Tensor
    n_meshes: int
    n_faces: int
    max_faces: int
    n_verts: int
    max_verts: int


def _point_mesh_inputs(who: str, verts: torch.Tensor, mt: MeshTables, points: torch.Tensor, lengths: Optional[torch.Tensor]):
    if verts.dtype != torch.float32 or points.dtype != torch.float32:
        raise ValueError(f"{who}: verts and points must be float32")
    if tuple(verts.shape) != (mt.n_verts, 3) or points.dim() != 3 or points.shape[0] != mt.n_meshes or points.shape[2] != 3:
        raise ValueError(f"{who}: verts ({mt.n_verts},3) packed and points ({mt.n_meshes},P,3), got {tuple(verts.shape)} and "
                         f"{tuple(points.shape)}")
    if mt.n_faces < 1 or points.shape[1] < 1:
        raise ValueError(f"{who}: needs at least one face and one point per cloud (F={mt.n_faces}, P={int(points.shape[1])})")
    if lengths is not None:
        if tuple(lengths.shape) != (mt.n_meshes,):
            raise ValueError(f"{who}: lengths ({mt.n_meshes},), got {tuple(lengths.shape)}")
        lengths = lengths.to(device=verts.device, dtype=torch.int32).contiguous()
    lib = _lib.checked()
    nbytes = int(lib.smil_point_mesh_workspace_bytes(mt.n_meshes, mt.n_faces, int(points.shape[1]), mt.n_verts))
    if nbytes == 0:
        raise _lib.SmilError(f"{who}: sizes N={mt.n_meshes} F={mt.n_faces} P={int(points.shape[1])} V={mt.n_verts} are not supported")
    return lib, verts.contiguous(), points.contiguous(), lengths, _workspace(nbytes, verts.device)


def point_mesh_distance(verts: torch.Tensor, mt: MeshTables, points: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                        by_face: bool = False, splits: int = 0):
    """The nearest face of its mesh for every point of points (N,P,3) (``by_face`` False: dist2 (N,P), face (N,P) int32, bary (N,P,3)),
    or the nearest point of its mesh's cloud for every face (True: dist2 (F_total), point (F_total) int32, bary (F_total,3) of the
    closest point on the face).  -1 and +inf where there is none.  ``splits``: 0 = automatic (smil_point_face_distance)."""
    who = "face_point_distance" if by_face else "point_face_distance"
    lib, verts, points, lengths, ws = _point_mesh_inputs(who, verts, mt, points, lengths)
    rows = (mt.n_faces,) if by_face else (mt.n_meshes, int(points.shape[1]))
    dist2 = torch.empty(rows, device=verts.device, dtype=torch.float32)
    idx = torch.empty(rows, device=verts.device, dtype=torch.int32)
    bary = torch.empty(rows + (3,), device=verts.device, dtype=torch.float32)
    fn = lib.smil_face_point_distance if by_face else lib.smil_point_face_distance
    fn(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), mt.n_meshes, mt.n_faces, mt.max_faces, _ptr(points), int(points.shape[1]),
       _ptr(lengths), int(splits), _ptr(dist2), _ptr(idx), _ptr(bary), _ptr(ws), _stream())
    return dist2, idx, bary


def point_mesh_backward(verts: torch.Tensor, mt: MeshTables, points: torch.Tensor, lengths: Optional[torch.Tensor], idx: torch.Tensor,
                        g: torch.Tensor, by_face: bool = False):
    """(d_points (N,P,3), d_verts (n_verts,3)) of sum_r g_r dist2_r over the records ``idx`` of one direction of point_mesh_distance."""
    lib, verts, points, lengths, ws = _point_mesh_inputs("point_mesh_backward", verts, mt, points, lengths)
    rows = (mt.n_faces,) if by_face else (mt.n_meshes, int(points.shape[1]))
    if tuple(idx.shape) != rows or idx.dtype != torch.int32 or tuple(g.shape) != rows or g.dtype != torch.float32:
        raise ValueError(f"point_mesh_backward: idx int32 and g float32 of shape {rows}")
    d_points = torch.empty_like(points)
    d_verts = torch.empty_like(verts)
    lib.smil_point_mesh_backward(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), _ptr(mt.vert_off), mt.n_meshes, mt.n_faces, mt.max_faces,
                                 mt.max_verts, _ptr(points), int(points.shape[1]), _ptr(lengths), int(bool(by_face)), _ptr(idx.contiguous()),
                                 _ptr(g.contiguous()), _ptr(d_points), _ptr(d_verts), _ptr(ws), _stream())
    return d_points, d_verts


def point_mesh_winding(verts: torch.Tensor, mt: MeshTables, points: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                       splits: int = 0) -> torch.Tensor:
    """The generalised winding number (N,P) float32 of every point of points (N,P,3) with respect to its mesh: the sum of the faces'
    signed solid angles / (4 pi) (smil_point_mesh_winding).  NaN for a point at or beyond its cloud's length or with an unusable
    coordinate.  ``splits``: 0 = automatic; every value gives the same bits.  No host synchronisation."""
    lib, verts, points, lengths, ws = _point_mesh_inputs("point_mesh_winding", verts, mt, points, lengths)
    winding = torch.empty((mt.n_meshes, int(points.shape[1])), device=verts.device, dtype=torch.float32)
    lib.smil_point_mesh_winding(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), mt.n_meshes, mt.n_faces, mt.max_faces, _ptr(points),
                                int(points.shape[1]), _ptr(lengths), int(splits), _ptr(winding), _ptr(ws), _stream())
    return winding


# ---- the face hierarchy of packed meshes (mesh_bvh.hip) ------------------------------------------------------------------------
def _bvh_inputs(who: str, verts: torch.Tensor, mt: MeshTables, P: int = 1):
    if verts.dtype != torch.float32 or tuple(verts.shape) != (mt.n_verts, 3):
        raise ValueError(f"{who}: verts ({mt.n_verts},3) packed float32, got {tuple(verts.shape)} {verts.dtype}")
    if mt.n_faces < 1:
        raise ValueError(f"{who}: needs at least one face (F={mt.n_faces})")
    lib = _lib.checked()
    nbytes = int(lib.smil_bvh_workspace_bytes(mt.n_meshes, mt.n_faces, P, mt.n_verts))
    if nbytes == 0:
        raise _lib.SmilError(f"{who}: sizes N={mt.n_meshes} F={mt.n_faces} P={P} V={mt.n_verts} are not supported")
    return lib, verts.contiguous(), _workspace(nbytes, verts.device)


def bvh_build(verts: torch.Tensor, mt: MeshTables):
    """(order (F_total) int32, boxes (nodes,6) float32) of the meshes' face hierarchies (smil_bvh_codes, a stable torch.sort of the
    int64 keys, smil_bvh_build).  No host synchronisation."""
    lib, verts, ws = _bvh_inputs("bvh_build", verts, mt)
    keys = torch.empty(mt.n_faces, device=verts.device, dtype=torch.int64)
    lib.smil_bvh_codes(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), mt.n_meshes, mt.n_faces, mt.max_faces, _ptr(keys), _ptr(ws),
                       _stream())
    perm = torch.sort(keys, stable=True).indices.contiguous()
    order = torch.empty(mt.n_faces, device=verts.device, dtype=torch.int32)
    # (zeros: the rows that no node owns - row 0 of every mesh, the padding to the next - are never written)
    boxes = torch.zeros((int(lib.smil_bvh_nodes(mt.n_meshes, mt.n_faces)), 6), device=verts.device, dtype=torch.float32)
    lib.smil_bvh_build(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), mt.n_meshes, mt.n_faces, mt.max_faces, _ptr(perm), _ptr(order),
                       _ptr(boxes), _ptr(ws), _stream())
    return order, boxes


def bvh_refit(verts: torch.Tensor, mt: MeshTables, order: torch.Tensor, boxes: torch.Tensor) -> None:
    """The boxes of ``bvh_build`` once more, in place, from new vertices in the stored order (smil_bvh_refit)."""
    lib, verts, ws = _bvh_inputs("bvh_refit", verts, mt)
    lib.smil_bvh_refit(_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), mt.n_meshes, mt.n_faces, mt.max_faces, _ptr(order), _ptr(boxes),
                       _ptr(ws), _stream())


def bvh_point_face_distance(verts: torch.Tensor, mt: MeshTables, order: torch.Tensor, boxes: torch.Tensor, points: torch.Tensor,
                            lengths: Optional[torch.Tensor] = None, sort_queries: bool = False, want_evaluated: bool = False):
    """``point_mesh_distance`` (points -> faces) through the hierarchy: the same dist2 (N,P), face (N,P) int32 and bary (N,P,3), bit for
    bit, and with ``want_evaluated`` the number of leaf faces evaluated per point (N,P) int32 (else None).  ``sort_queries``: the
    lanes of a wave take points that are neighbours in space (smil_bvh_point_codes, a stable sort, the results scattered back): the
    same answers, other timings."""
    who = "bvh_point_face_distance"
    _, verts, points, lengths, _ = _point_mesh_inputs(who, verts, mt, points, lengths)
    N, P = mt.n_meshes, int(points.shape[1])
    lib, verts, ws = _bvh_inputs(who, verts, mt, P)
    if tuple(order.shape) != (mt.n_faces,) or order.dtype != torch.int32 or boxes.dtype != torch.float32 or \
            tuple(boxes.shape) != (int(lib.smil_bvh_nodes(N, mt.n_faces)), 6):
        raise ValueError(f"{who}: order and boxes are not a hierarchy of these meshes")
    mesh = (_ptr(verts), mt.n_verts, _ptr(mt.faces), _ptr(mt.face_off), N, mt.n_faces, mt.max_faces)
    back = None
    if sort_queries:
        keys = torch.empty((N, P), device=verts.device, dtype=torch.int64)
        lib.smil_bvh_point_codes(*mesh, _ptr(boxes), _ptr(points), P, _ptr(lengths), _ptr(keys), _ptr(ws), _stream())
        back = torch.sort(keys, dim=1, stable=True).indices  # (padded and unusable points sort behind the cloud, in their order)
        points = torch.gather(points, 1, back[:, :, None].expand(N, P, 3)).contiguous()
    dist2 = torch.empty((N, P), device=verts.device, dtype=torch.float32)
    face = torch.empty((N, P), device=verts.device, dtype=torch.int32)
    bary = torch.empty((N, P, 3), device=verts.device, dtype=torch.float32)
    evaluated = torch.empty((N, P), device=verts.device, dtype=torch.int32) if want_evaluated else None
    lib.smil_bvh_point_face_distance(*mesh, _ptr(order), _ptr(boxes), _ptr(points), P, _ptr(lengths), _ptr(dist2), _ptr(face), _ptr(bary),
                                     _ptr(evaluated), _ptr(ws), _stream())
    if back is not None:
        dist2, face = torch.empty_like(dist2).scatter_(1, back, dist2), torch.empty_like(face).scatter_(1, back, face)
        bary = torch.empty_like(bary).scatter_(1, back[:, :, None].expand(N, P, 3), bary)
        if evaluated is not None:
            evaluated = torch.empty_like(evaluated).scatter_(1, back, evaluated)
    return dist2, face, bary, evaluated


# ---- PointNet++ set-abstraction operations (pointnet2.hip) ---------------------------------------------------------------------
def _check_cloud(what: str, name: str, t: torch.Tensor, B: Optional[int] = None, last: Optional[int] = 3) -> None:
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.float32 and (last is None or t.shape[2] == last)
            and (B is None or t.shape[0] == B)):
        raise ValueError(f"{what}: {name} must be a float32 tensor (B, n, {'D' if last is None else last})")


def fps(xyz: torch.Tensor, npoint: int, start: torch.Tensor) -> torch.Tensor:
    """Farthest point sampling of xyz (B,N,3) from the start indices (B) int32: (B,npoint) int32 (smil_fps, include/smilfit.h).
    ValueError when N exceeds SMIL_FPS_MAX_N."""
    _check_cloud("fps", "xyz", xyz)
    B, N, npoint = int(xyz.shape[0]), int(xyz.shape[1]), int(npoint)
    if start.dtype != torch.int32 or tuple(start.shape) != (B,):
        raise ValueError("fps: start must be an int32 tensor (B)")
    if N > _lib.FPS_MAX_N:
        raise ValueError(f"fps: N={N} above SMIL_FPS_MAX_N={_lib.FPS_MAX_N}")
    if B < 1 or N < 1 or npoint < 1:
        raise ValueError(f"fps: bad sizes B={B} N={N} npoint={npoint}")
    xyz, start = xyz.contiguous(), start.contiguous()
    out = torch.empty(B, npoint, device=xyz.device, dtype=torch.int32)
    _lib.checked().smil_fps(_ptr(xyz), _ptr(start), B, N, npoint, _ptr(out), _stream())
    return out


def ball_query(xyz: torch.Tensor, new_xyz: torch.Tensor, radii, nsamples):
    """The ball queries of new_xyz (B,S,3) in xyz (B,N,3) at 1 .. SMIL_BALL_MAX_RADII (radius, nsample) pairs in one launch: a list of
    (B,S,min(nsample, N)) int32 index tensors (smil_ball_query, include/smilfit.h)."""
    _check_cloud("ball_query", "xyz", xyz)
    _check_cloud("ball_query", "new_xyz", new_xyz, B=int(xyz.shape[0]))
    radii, nsamples = [float(r) for r in radii], [int(k) for k in nsamples]
    n = len(radii)
    if not 1 <= n <= _lib.BALL_MAX_RADII or len(nsamples) != n:
        raise ValueError(f"ball_query: 1 .. {_lib.BALL_MAX_RADII} (radius, nsample) pairs, got {n} radii and {len(nsamples)} nsample")
    if min(nsamples) < 1 or not all(np.isfinite(r) and r >= 0.0 for r in radii):
        raise ValueError(f"ball_query: nsample >= 1 and finite radii >= 0 (got {nsamples}, {radii})")
    B, N, S = int(xyz.shape[0]), int(xyz.shape[1]), int(new_xyz.shape[1])
    if B < 1 or N < 1 or S < 1:
        raise ValueError(f"ball_query: bad sizes B={B} N={N} S={S}")
    xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
    outs = [torch.empty(B, S, min(k, N), device=xyz.device, dtype=torch.int32) for k in nsamples]
    _lib.checked().smil_ball_query(_ptr(xyz), _ptr(new_xyz), B, N, S, n, (ctypes.c_double * n)(*radii), (ctypes.c_int32 * n)(*nsamples),
                                   (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), _stream())
    return outs


def group_points(xyz: Optional[torch.Tensor], centres: Optional[torch.Tensor], features: Optional[torch.Tensor], idx: torch.Tensor,
                 xyz_last: bool = False) -> torch.Tensor:
    """The grouped tensor (B,C,K,S) of idx (B,S,K) int32: channels [xyz - centres (3), features (D)], or [features, xyz - centres]
    with ``xyz_last``; xyz None: features only, centres None: coordinates as they are (smil_group_points, include/smilfit.h)."""
    if xyz is None and features is None:
        raise ValueError("group_points: neither coordinates nor features")
    if idx.dim() != 3 or idx.dtype != torch.int32:
        raise ValueError("group_points: idx must be an int32 tensor (B, S, K)")
    B, S, K = (int(v) for v in idx.shape)
    src = xyz if xyz is not None else features
    N = int(src.shape[1]) if src.dim() == 3 else 0
    if xyz is not None:
        _check_cloud("group_points", "xyz", xyz, B=B)
    if centres is not None:
        _check_cloud("group_points", "centres", centres, B=B)
        if xyz is None or int(centres.shape[1]) != S:
            raise ValueError("group_points: centres (B, S, 3) need xyz and one centre per query")
    D = 0
    if features is not None:
        _check_cloud("group_points", "features", features, B=B, last=None)
        D = int(features.shape[2])
        if int(features.shape[1]) != N:
            raise ValueError("group_points: features (B, N, D) and xyz (B, N, 3) differ in N")
    if min(B, S, K, N) < 1 or (xyz is None and D < 1):
        raise ValueError(f"group_points: bad sizes B={B} N={N} S={S} K={K} D={D}")
    xyz, centres, features, idx = (None if t is None else t.contiguous() for t in (xyz, centres, features, idx))
    out = torch.empty(B, (0 if xyz is None else 3) + D, K, S, device=idx.device, dtype=torch.float32)
    _lib.checked().smil_group_points(_ptr(xyz), _ptr(centres), _ptr(features if D else None), _ptr(idx), B, N, S, K, D, int(bool(xyz_last)),
                                     _ptr(out), _stream())
    return out


def group_points_backward(d_out: torch.Tensor, idx: torch.Tensor, N: int, D: int, has_xyz: bool, xyz_last: bool) -> torch.Tensor:
    """d_features (B,N,D): d_out (B,C,K,S)'s feature channels summed over the positions that drew each point (order-independent)."""
    B, S, K = (int(v) for v in idx.shape)
    N, D = int(N), int(D)
    if idx.dtype != torch.int32 or d_out.dtype != torch.float32 or tuple(d_out.shape) != (B, (3 if has_xyz else 0) + D, K, S) or D < 1:
        raise ValueError("group_points_backward: d_out (B, C, K, S) float32 and idx (B, S, K) int32 with C = 3 + D or D >= 1")
    d_out, idx = d_out.contiguous(), idx.contiguous()
    lib = _lib.checked()
    ws = _workspace(lib.smil_group_points_backward_workspace_bytes(B, N, D), d_out.device)
    d_feat = torch.empty(B, N, D, device=d_out.device, dtype=torch.float32)
    lib.smil_group_points_backward(_ptr(d_out), _ptr(idx), B, N, S, K, D, int(bool(has_xyz)), int(bool(xyz_last)), _ptr(d_feat), _ptr(ws), _stream())
    return d_feat


def upload_f64(x, device):
    """x (array-like or None) as a contiguous float64 tensor on device: how the numpy-level wrappers hand arrays to the functions below."""
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(device)


def _require_f64(who, name, t, shape, device):
    """t contiguous, or the ValueError of the multi-view entry points for a tensor that is not float64 of this shape on this device."""
    if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != device:
        raise ValueError(f"{who}: {name} must be a float64 tensor {shape} on {device}")
    return t.contiguous()


def triangulate(P: torch.Tensor, obs: torch.Tensor, scores: Optional[torch.Tensor], pairs: Optional[torch.Tensor], *,
                K: Optional[torch.Tensor] = None, dist: Optional[torch.Tensor] = None, confidence_threshold: float = 0.3,
                min_views: int = 2, reproj_threshold: float = 15.0, mode: int = _lib.TRI_RANSAC, want_view_err: bool = False,
                want_inlier_mask: bool = False, want_undistorted: bool = False):
    """DLT / pair-RANSAC triangulation of obs (N,Kp,C,2) float64 through P (C,3,4) float64 (smil_triangulate, include/smilfit.h):
    ``(xyz (N,Kp,3), status (N,Kp) int32, views_used (N,Kp) int32, mean_err (N,Kp), view_err (N,Kp,C) or None, inlier_mask (N,Kp)
    int32 bits or None, obs_undistorted (N,Kp,C,2) or None: NaN for a dropped view)``.  scores (N,Kp,C) or None; K (C,3,3) and dist (C,5) together or not at all; pairs: the hypothesis table
    (SMIL_TRI_MAX_VIEWS + 1, SMIL_TRI_MAX_HYP, 2) int32, needed with ``mode & TRI_RANSAC``.  ValueError above SMIL_TRI_MAX_VIEWS."""
    if obs.dim() != 4 or obs.shape[3] != 2 or obs.dtype != torch.float64:
        raise ValueError("triangulate: obs must be a float64 tensor (N, Kp, C, 2)")
    require_gpu(obs.device)
    N, Kp, C = (int(v) for v in obs.shape[:3])
    if C > _lib.TRI_MAX_VIEWS:
        raise ValueError(f"triangulate: C={C} cameras above SMIL_TRI_MAX_VIEWS={_lib.TRI_MAX_VIEWS}")
    if min(N, Kp, C) < 1 or int(min_views) < 1:
        raise ValueError(f"triangulate: bad sizes N={N} Kp={Kp} C={C} min_views={min_views}")

    f64 = lambda name, t, shape: None if t is None else _require_f64("triangulate", name, t, shape, obs.device)  # noqa: E731
    P, K, dist = f64("P", P, (C, 3, 4)), f64("K", K, (C, 3, 3)), f64("dist", dist, (C, 5))
    scores = f64("scores", scores, (N, Kp, C))
    if P is None or (K is None) != (dist is None):
        raise ValueError("triangulate: P is required, and K and dist come together")
    if mode & _lib.TRI_RANSAC:
        if pairs is None or pairs.dtype != torch.int32 or tuple(pairs.shape) != (_lib.TRI_MAX_VIEWS + 1, _lib.TRI_MAX_HYP, 2) \
                or pairs.device != obs.device:
            raise ValueError("triangulate: RANSAC needs the int32 pair table (SMIL_TRI_MAX_VIEWS + 1, SMIL_TRI_MAX_HYP, 2)")
        pairs = pairs.contiguous()
    obs = obs.contiguous()
    dev = obs.device
    xyz = torch.empty(N, Kp, 3, device=dev, dtype=torch.float64)
    status = torch.empty(N, Kp, device=dev, dtype=torch.int32)
    used = torch.empty(N, Kp, device=dev, dtype=torch.int32)
    mean_err = torch.empty(N, Kp, device=dev, dtype=torch.float64)
    view_err = torch.empty(N, Kp, C, device=dev, dtype=torch.float64) if want_view_err else None
    mask = torch.empty(N, Kp, device=dev, dtype=torch.int32) if want_inlier_mask else None
    undist = torch.full((N, Kp, C, 2), float("nan"), device=dev, dtype=torch.float64) if want_undistorted else None
    _lib.checked().smil_triangulate(_ptr(P), _ptr(K), _ptr(dist), _ptr(obs), _ptr(scores), _ptr(pairs), N, Kp, C, float(confidence_threshold),
                                    int(min_views), float(reproj_threshold), int(mode), _ptr(xyz), _ptr(status), _ptr(used), _ptr(mean_err),
                                    _ptr(view_err), _ptr(mask), _ptr(undist), _stream())
    return xyz, status, used, mean_err, view_err, mask, undist


def _refine_inputs(who, pts_3d, pts_2d, offsets, params, n_params, f_scale):
    """Shared checks of the two refinement entry points; offsets is a host int64 array (C + 1).  Returns the contiguous tensors, the
    device copy of the offsets and a workspace."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    if offsets.ndim != 1 or len(offsets) < 2 or offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError(f"{who}: offsets must be a non-decreasing int64 table (C + 1) that starts at 0")
    C, total = len(offsets) - 1, int(offsets[-1])
    require_gpu(params.device)
    pts_3d, pts_2d, params = (_require_f64(who, name, t, shape, params.device) for name, t, shape in
                              (("pts_3d", pts_3d, (total, 3)), ("pts_2d", pts_2d, (total, 2)), ("params", params, (C, 10))))
    if int(n_params) not in (6, 10) or not float(f_scale) > 0.0:
        raise ValueError(f"{who}: n_params={n_params} must be 6 or 10 and f_scale={f_scale} positive")
    lib = _lib.checked()
    ws = _workspace(lib.smil_refine_workspace_bytes(C, int(np.diff(offsets).max())), params.device)
    return pts_3d, pts_2d, params, offsets, torch.from_numpy(offsets).to(params.device), C, ws


def refine_evaluate(pts_3d: torch.Tensor, pts_2d: torch.Tensor, offsets, params: torch.Tensor, *, n_params: int = 10,
                    f_scale: float = 5.0):
    """One accumulation of the camera refinement (smil_refine_evaluate, include/smilfit.h) at params (C,10) float64 over the packed
    correspondences pts_3d (sum M,3), pts_2d (sum M,2) with the host table offsets (C+1): ``(cost (C), g (C,10), H (C,10,10))``."""
    pts_3d, pts_2d, params, offsets, off_dev, C, ws = _refine_inputs("refine_evaluate", pts_3d, pts_2d, offsets, params, n_params, f_scale)
    dev = params.device
    cost = torch.empty(C, device=dev, dtype=torch.float64)
    g = torch.empty(C, 10, device=dev, dtype=torch.float64)
    H = torch.empty(C, 10, 10, device=dev, dtype=torch.float64)
    _lib.checked().smil_refine_evaluate(_ptr(pts_3d), _ptr(pts_2d), offsets.ctypes.data, _ptr(off_dev), C, _ptr(params), int(n_params),
                                        float(f_scale), _ptr(cost), _ptr(g), _ptr(H), _ptr(ws), _stream())
    return cost, g, H


def refine_cameras(pts_3d: torch.Tensor, pts_2d: torch.Tensor, offsets, params0: torch.Tensor, *, n_params: int = 10, f_scale: float = 5.0,
                   max_steps: int = 100):
    """Robust Levenberg-Marquardt of every camera's parameters (smil_refine_cameras, include/smilfit.h): ``(params (C,10), status (C)
    int32, n_accepted (C) int32, n_trials (C) int32, cost0 (C), cost (C), g (C,10))``.  Synchronises the current stream."""
    if int(max_steps) < 1:
        raise ValueError(f"refine_cameras: max_steps={max_steps} must be >= 1")
    pts_3d, pts_2d, params0, offsets, off_dev, C, ws = _refine_inputs("refine_cameras", pts_3d, pts_2d, offsets, params0, n_params, f_scale)
    dev = params0.device
    params = torch.empty(C, 10, device=dev, dtype=torch.float64)
    status, n_acc, n_trial = (torch.empty(C, device=dev, dtype=torch.int32) for _ in range(3))
    cost0, cost = (torch.empty(C, device=dev, dtype=torch.float64) for _ in range(2))
    g = torch.empty(C, 10, device=dev, dtype=torch.float64)
    _lib.checked().smil_refine_cameras(_ptr(pts_3d), _ptr(pts_2d), offsets.ctypes.data, _ptr(off_dev), C, _ptr(params0), int(n_params),
                                       float(f_scale), int(max_steps), _ptr(params), _ptr(status), _ptr(n_acc), _ptr(n_trial), _ptr(cost0),
                                       _ptr(cost), _ptr(g), _ptr(ws), _stream())
    return params, status, n_acc, n_trial, cost0, cost, g


def _refine_points_inputs(who, P, obs, view_mask, xyz, f_scale):
    """Shared checks of the two point refinement entry points.  Returns the contiguous tensors and N, Kp, C."""
    if obs.dim() != 4 or obs.shape[3] != 2 or obs.dtype != torch.float64:
        raise ValueError(f"{who}: obs must be a float64 tensor (N, Kp, C, 2)")
    require_gpu(obs.device)
    N, Kp, C = (int(v) for v in obs.shape[:3])
    if not 1 <= C <= _lib.TRI_MAX_VIEWS:
        raise ValueError(f"{who}: C={C} cameras outside 1 .. SMIL_TRI_MAX_VIEWS={_lib.TRI_MAX_VIEWS}")
    P, xyz = _require_f64(who, "P", P, (C, 3, 4), obs.device), _require_f64(who, "xyz", xyz, (N, Kp, 3), obs.device)
    if view_mask.dtype != torch.int32 or tuple(view_mask.shape) != (N, Kp) or view_mask.device != obs.device:
        raise ValueError(f"{who}: view_mask must be an int32 tensor {(N, Kp)} of bits on {obs.device}")
    if not float(f_scale) > 0.0:
        raise ValueError(f"{who}: f_scale={f_scale} must be positive")
    return P, obs.contiguous(), view_mask.contiguous(), xyz, N, Kp, C


def refine_points_evaluate(P: torch.Tensor, obs: torch.Tensor, view_mask: torch.Tensor, xyz: torch.Tensor, *, f_scale: float = 5.0):
    """One accumulation of the point refinement (smil_refine_points_evaluate, include/smilfit.h) at xyz (N,Kp,3) float64 over the views
    of view_mask (N,Kp) int32 bits of obs (N,Kp,C,2) through P (C,3,4): ``(cost (N,Kp), g (N,Kp,3), H (N,Kp,3,3))``."""
    P, obs, view_mask, xyz, N, Kp, C = _refine_points_inputs("refine_points_evaluate", P, obs, view_mask, xyz, f_scale)
    dev = obs.device
    cost = torch.empty(N, Kp, device=dev, dtype=torch.float64)
    g = torch.empty(N, Kp, 3, device=dev, dtype=torch.float64)
    H = torch.empty(N, Kp, 3, 3, device=dev, dtype=torch.float64)
    _lib.checked().smil_refine_points_evaluate(_ptr(P), _ptr(obs), _ptr(view_mask), _ptr(xyz), N, Kp, C, float(f_scale), _ptr(cost), _ptr(g), _ptr(H),
                                               _stream())
    return cost, g, H


def refine_points(P: torch.Tensor, obs: torch.Tensor, view_mask: torch.Tensor, xyz0: torch.Tensor, *, f_scale: float = 5.0,
                  max_steps: int = 50, want_view_err: bool = False):
    """Robust Levenberg-Marquardt of every point over its views (smil_refine_points, include/smilfit.h): ``(xyz (N,Kp,3), status (N,Kp)
    int32, n_accepted (N,Kp) int32, n_trials (N,Kp) int32, cost0 (N,Kp), cost (N,Kp), view_err (N,Kp,C) or None)``.  Asynchronous."""
    if int(max_steps) < 1:
        raise ValueError(f"refine_points: max_steps={max_steps} must be >= 1")
    P, obs, view_mask, xyz0, N, Kp, C = _refine_points_inputs("refine_points", P, obs, view_mask, xyz0, f_scale)
    dev = obs.device
    xyz = torch.empty(N, Kp, 3, device=dev, dtype=torch.float64)
    status, n_acc, n_trial = (torch.empty(N, Kp, device=dev, dtype=torch.int32) for _ in range(3))
    cost0, cost = (torch.empty(N, Kp, device=dev, dtype=torch.float64) for _ in range(2))
    view_err = torch.empty(N, Kp, C, device=dev, dtype=torch.float64) if want_view_err else None
    _lib.checked().smil_refine_points(_ptr(P), _ptr(obs), _ptr(view_mask), _ptr(xyz0), N, Kp, C, float(f_scale), int(max_steps), _ptr(xyz),
                                      _ptr(status), _ptr(n_acc), _ptr(n_trial), _ptr(cost0), _ptr(cost), _ptr(view_err), _stream())
    return xyz, status, n_acc, n_trial, cost0, cost, view_err


# ---- target image preparation (csrc/imageprep.hip) ----
WARP_COORD_MODES = {"exact": _lib.WARP_EXACT, "resize_linear": _lib.WARP_RESIZE_LINEAR, "resize_nearest": _lib.WARP_RESIZE_NEAREST}
WARP_INTERPOLATIONS = {"nearest": _lib.WARP_NEAREST, "bilinear": _lib.WARP_BILINEAR}


def image_bounds(sil: torch.Tensor) -> torch.Tensor:
    """sil (N,H,W) uint8 or float32 -> (N,5) int32 ``y_min, y_max, x_min, x_max, count`` over the pixels > 0; an image without one
    keeps ``H, -1, W, -1, 0`` (smil_image_bounds, include/smilfit.h).  An exact integer reduction: two calls give the same bits."""
    if not isinstance(sil, torch.Tensor) or sil.dim() != 3 or sil.dtype not in (torch.uint8, torch.float32):
        raise ValueError("image_bounds: sil must be a uint8 or float32 tensor (N, H, W)")
    N, H, W = (int(v) for v in sil.shape)
    if H < 1 or W < 1 or H * W > 2**31 - 2**16 - 1:
        raise ValueError(f"image_bounds: images of {H} x {W} pixels cannot be indexed")
    dev = require_gpu(sil.device)
    sil = sil.contiguous()
    bounds = torch.empty(N, 5, dtype=torch.int32, device=dev)
    _lib.checked().smil_image_bounds(_ptr(sil), int(sil.dtype == torch.uint8), N, H, W, _ptr(bounds), _stream())
    return bounds


def _warp_table(name, t, row_shape, dtype, device):
    """A per-image table: (k, *row_shape) of dtype on device with k >= 1 (a single row may come without the leading axis)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"warp_images: {name} must be a {dtype} tensor (k, {', '.join(map(str, row_shape))})")
    if tuple(t.shape) == tuple(row_shape):
        t = t[None]
    if t.dim() != len(row_shape) + 1 or tuple(t.shape[1:]) != tuple(row_shape) or t.shape[0] < 1:
        raise ValueError(f"warp_images: {name} must be (k, {', '.join(map(str, row_shape))}) with k >= 1, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"warp_images: {name} must be on {device}, got {t.device}")
    return t.contiguous()


def warp_images(src: torch.Tensor, size, affine: torch.Tensor, *, coord_mode: str = "exact", interpolation: str = "bilinear",
                K: Optional[torch.Tensor] = None, K_new: Optional[torch.Tensor] = None, dist: Optional[torch.Tensor] = None,
                clamp: Optional[torch.Tensor] = None, border: Optional[torch.Tensor] = None, scale: float = 1.0, planar: bool = False,
                n_out: Optional[int] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One resampling of ``n_out`` images of ``size = (S_h, S_w)`` from ``src`` (N_src,H,W,C) channels-last or (N_src,H,W), uint8 or
    float32, C in 1 .. 4 (smil_warp_images, include/smilfit.h, states the map to the bit).  Output image n reads source image
    ``n % N_src`` and row ``n % k`` of every table: ``affine`` (k,4) float64 = ``ax, bx, ay, by``; ``K``, ``K_new`` (k,3,3) and
    ``dist`` (k,5) float64, all three or none (``coord_mode="exact"`` only); ``clamp`` (k,4) int32 = ``x_lo, x_hi, y_lo, y_hi`` or
    None; ``border`` (k,C) float32, None: zeros.  ``n_out`` defaults to the longest of N_src and the tables.  Returns float32 (or, with
    ``out_dtype=torch.uint8``, the rounded and clipped bytes) ``(N,S_h,S_w,C)`` - without the channel axis for a 3-D ``src`` - or with
    ``planar`` ``(N,C,S_h,S_w)``.  Everything is checked before the device is touched."""
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4) or src.dtype not in (torch.uint8, torch.float32):
        raise ValueError("warp_images: src must be a uint8 or float32 tensor (N_src, H, W, C) or (N_src, H, W)")
    has_c = src.dim() == 4
    N_src, H, W = (int(v) for v in src.shape[:3])
    C = int(src.shape[3]) if has_c else 1
    if not 1 <= C <= 4:
        raise ValueError(f"warp_images: C={C} channels, 1 to 4 are supported")
    if N_src < 1 or H < 1 or W < 1 or H >= 2**30 or W >= 2**30:
        raise ValueError(f"warp_images: bad source sizes N_src={N_src} H={H} W={W}")
    try:
        S_h, S_w = (int(v) for v in size)
    except TypeError:
        S_h = S_w = int(size)
    if S_h < 1 or S_w < 1 or S_h * S_w > 2**31 - 257:
        raise ValueError(f"warp_images: bad output size {S_h} x {S_w}")
    if coord_mode not in WARP_COORD_MODES or interpolation not in WARP_INTERPOLATIONS:
        raise ValueError(f"warp_images: coord_mode is one of {sorted(WARP_COORD_MODES)} and interpolation one of "
                         f"{sorted(WARP_INTERPOLATIONS)}, got {coord_mode!r} and {interpolation!r}")
    own = {"resize_linear": "bilinear", "resize_nearest": "nearest"}.get(coord_mode)
    if own is not None and interpolation != own:
        raise ValueError(f"warp_images: coord_mode {coord_mode!r} goes with interpolation {own!r}")
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"warp_images: out_dtype must be float32 or uint8, got {out_dtype}")
    dev = src.device
    affine = _warp_table("affine", affine, (4,), torch.float64, dev)
    if affine is None:
        raise ValueError("warp_images: affine is required")
    lens = [K, K_new, dist]
    if any(t is not None for t in lens) and any(t is None for t in lens):
        raise ValueError("warp_images: K, K_new and dist come together")
    K, K_new = _warp_table("K", K, (3, 3), torch.float64, dev), _warp_table("K_new", K_new, (3, 3), torch.float64, dev)
    dist = _warp_table("dist", dist, (5,), torch.float64, dev)
    if K is not None:
        if coord_mode != "exact":
            raise ValueError("warp_images: a lens needs coord_mode='exact'")
        if not (K.shape[0] == K_new.shape[0] == dist.shape[0]):
            raise ValueError(f"warp_images: K, K_new and dist must have the same number of rows, got {K.shape[0]}, {K_new.shape[0]}, {dist.shape[0]}")
    clamp = _warp_table("clamp", clamp, (4,), torch.int32, dev)
    if border is None:
        border = torch.zeros(1, C, dtype=torch.float32, device=dev)
    border = _warp_table("border", border, (C,), torch.float32, dev)
    tables = [affine.shape[0], border.shape[0]] + ([K.shape[0]] if K is not None else []) + ([clamp.shape[0]] if clamp is not None else [])
    N = max([N_src] + tables) if n_out is None else int(n_out)
    if N < 0 or N * ((S_h * S_w + 255) // 256) > 2**31 - 1:
        raise ValueError(f"warp_images: {N} output images of {S_h} x {S_w} pixels cannot be launched in one call")
    dev = require_gpu(dev)
    src = src.contiguous()
    shape = (N, C, S_h, S_w) if planar else ((N, S_h, S_w, C) if has_c else (N, S_h, S_w))
    out = torch.empty(shape, dtype=out_dtype, device=dev)
    w = _lib.Warp()
    w.src, w.src_is_u8, w.N_src, w.H, w.W, w.C = src.data_ptr(), int(src.dtype == torch.uint8), N_src, H, W, C
    w.out, w.out_is_u8, w.planar, w.N, w.S_h, w.S_w = out.data_ptr(), int(out_dtype == torch.uint8), int(bool(planar)), N, S_h, S_w
    w.coord_mode, w.interp = WARP_COORD_MODES[coord_mode], WARP_INTERPOLATIONS[interpolation]
    w.affine, w.n_affine = affine.data_ptr(), int(affine.shape[0])
    if K is not None:
        w.K, w.K_new, w.dist, w.n_lens = K.data_ptr(), K_new.data_ptr(), dist.data_ptr(), int(K.shape[0])
    if clamp is not None:
        w.clamp, w.n_clamp = clamp.data_ptr(), int(clamp.shape[0])
    w.border, w.n_border, w.scale = border.data_ptr(), int(border.shape[0]), float(scale)
    _lib.checked().smil_warp_images(ctypes.byref(w), _stream())
    return out


# ---- rotation conversions (csrc/rotations.hip) ----
ROT_DTYPES = {torch.float32: _lib.ROT_F32, torch.float64: _lib.ROT_F64}


def rot_call(name: str, n: int, dtype: torch.dtype, *tensors: Optional[torch.Tensor]) -> None:
    """One ``smil_*`` rotation entry point over ``n`` rotations: the tensors in the order of its pointer arguments (None: NULL)."""
    getattr(_lib.checked(), name)(*(_ptr(t) for t in tensors), int(n), ROT_DTYPES[dtype], _stream())


def rot_forward(name: str, x: torch.Tensor, width: int) -> torch.Tensor:
    """``x`` (n,k) contiguous float32 / float64 on the GPU -> (n,width) through the forward entry point ``name``."""
    out = torch.empty(x.shape[0], width, dtype=x.dtype, device=x.device)
    rot_call(name, x.shape[0], x.dtype, x, out)
    return out


def rot_backward(name: str, x: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    """The gradient on ``x`` (n,k) from the upstream ``grad`` (n,width) through the backward entry point ``name``."""
    dx = torch.empty_like(x)
    rot_call(name, x.shape[0], x.dtype, x, grad, dx)
    return dx


def rot6d_distance(p6: torch.Tensor, t6: torch.Tensor) -> torch.Tensor:
    """(n,6), (n,6) -> (n,) Frobenius distances of the two rotations' matrices."""
    dist = torch.empty(p6.shape[0], dtype=p6.dtype, device=p6.device)
    rot_call("smil_rot6d_distance", p6.shape[0], p6.dtype, p6, t6, dist)
    return dist


def rot6d_distance_backward(p6: torch.Tensor, t6: torch.Tensor, ddist: torch.Tensor, need_p: bool = True, need_t: bool = True):
    """``(dp6, dt6)``, each (n,6) or None where it is not needed."""
    dp = torch.empty_like(p6) if need_p else None
    dt = torch.empty_like(t6) if need_t else None
    if need_p or need_t:
        rot_call("smil_rot6d_distance_backward", p6.shape[0], p6.dtype, p6, t6, ddist, dp, dt)
    return dp, dt


# ---- keypoint and triangulation losses (csrc/keypoint_losses.hip) ----
# Every tensor below is contiguous on one GPU: floats in one storage type of ROT_DTYPES, visibility and masks uint8 (or None), joint
# weights float64 (or None).  Scalars (losses, their upstream gradients) are 0-dim device tensors: nothing here synchronises.
KP_REDUCTIONS = {"pooled": _lib.KP_POOLED, "valid_samples": _lib.KP_VALID_SAMPLES, "samples": _lib.KP_SAMPLES}
KP_FLAGS_2D = _lib.KP_TARGET_IN_UNIT | _lib.KP_PRED_NAN_TO_ZERO
KP_FLAGS_3D = _lib.KP_FINITE_NONZERO


def _kp_f64(*shape, device) -> torch.Tensor:
    return torch.empty(*shape, dtype=torch.float64, device=device)


def kp_se_forward(pred: torch.Tensor, target: torch.Tensor, vis, mask, weights, flags: int, rule: int):
    """``pred``, ``target`` (N,J,D) -> ``(loss (), factor (N) float64)``: smil_kp_se_forward."""
    N, J, D = pred.shape
    loss = torch.empty((), dtype=pred.dtype, device=pred.device)
    factor = _kp_f64(N, device=pred.device)
    _lib.checked().smil_kp_se_forward(_ptr(pred), _ptr(target), _ptr(vis), _ptr(mask), _ptr(weights), N, J, D, flags, rule, ROT_DTYPES[pred.dtype],
                                      _ptr(_kp_f64(N, 4, device=pred.device)), _ptr(factor), _ptr(loss), _stream())
    return loss, factor


def kp_se_backward(pred, target, vis, mask, weights, factor, upstream: torch.Tensor, flags: int) -> torch.Tensor:
    """The gradient on ``pred`` from the 0-dim device tensor ``upstream``."""
    N, J, D = pred.shape
    dpred = torch.empty_like(pred)
    _lib.checked().smil_kp_se_backward(_ptr(pred), _ptr(target), _ptr(vis), _ptr(mask), _ptr(weights), _ptr(factor), _ptr(upstream), _ptr(dpred), N,
                                       J, D, flags, ROT_DTYPES[pred.dtype], _stream())
    return dpred


def _kp_sizes(R: torch.Tensor, J: int):
    return int(R.shape[0]), int(R.shape[1]), int(J)


def kp_project(joints, R, T, fov, aspect, S: float) -> torch.Tensor:
    """joints (B,J,3), R (B,V,3,3), T (B,V,3), fov (B,V), aspect (B,V) or None -> (B,V,J,2) normalised, clamped (y, x)."""
    B, V, J = _kp_sizes(R, joints.shape[1])
    out = torch.empty(B, V, J, 2, dtype=joints.dtype, device=joints.device)
    _lib.checked().smil_kp_project(_ptr(joints), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), B, V, J, float(S), ROT_DTYPES[joints.dtype], _ptr(out),
                                   _stream())
    return out


def _kp_camera_grads(joints, R, T, fov, need):
    """Output buffers (d joints, d R, d T, d fov), None where ``need`` says nobody wants it."""
    return tuple(torch.empty_like(t) if n else None for t, n in zip((joints, R, T, fov), need))


def kp_project_backward(joints, R, T, fov, aspect, dout, S: float, need=(True, True, True, True)):
    B, V, J = _kp_sizes(R, joints.shape[1])
    grads = _kp_camera_grads(joints, R, T, fov, need)
    if any(need):
        _lib.checked().smil_kp_project_backward(_ptr(joints), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), _ptr(dout), B, V, J, float(S),
                                                ROT_DTYPES[joints.dtype], *(_ptr(g) for g in grads), _stream())
    return grads


def kp_project_loss(joints, R, T, fov, aspect, target, vis, view_mask, weights, S: float):
    """The pooled 2-D loss of the projections against target (B,V,J,2) -> ``(loss (), factor (B V) float64)``."""
    B, V, J = _kp_sizes(R, joints.shape[1])
    loss = torch.empty((), dtype=joints.dtype, device=joints.device)
    factor = _kp_f64(B * V, device=joints.device)
    _lib.checked().smil_kp_project_loss(_ptr(joints), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), _ptr(target), _ptr(vis), _ptr(view_mask),
                                        _ptr(weights), B, V, J, float(S), ROT_DTYPES[joints.dtype], _ptr(_kp_f64(B * V, 4, device=joints.device)),
                                        _ptr(factor), _ptr(loss), _stream())
    return loss, factor


def kp_project_loss_backward(joints, R, T, fov, aspect, target, vis, view_mask, weights, factor, upstream, S: float,
                             need=(True, True, True, True)):
    B, V, J = _kp_sizes(R, joints.shape[1])
    grads = _kp_camera_grads(joints, R, T, fov, need)
    if any(need):
        _lib.checked().smil_kp_project_loss_backward(_ptr(joints), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), _ptr(target), _ptr(vis),
                                                     _ptr(view_mask), _ptr(weights), _ptr(factor), _ptr(upstream), B, V, J, float(S),
                                                     ROT_DTYPES[joints.dtype], *(_ptr(g) for g in grads), _stream())
    return grads


def kp_triangulate(kp, vis, view_mask, R, T, fov, aspect, S: float, damping: float, max_norm: Optional[float] = None):
    """kp (B,V,J,2) -> ``(points (B,J,3), valid (B,J) uint8, sane (B,J) uint8 or None)``; ``sane`` = valid and |point| < max_norm."""
    B, V, J = _kp_sizes(R, kp.shape[2])
    points = torch.empty(B, J, 3, dtype=kp.dtype, device=kp.device)
    valid = torch.empty(B, J, dtype=torch.uint8, device=kp.device)
    sane = torch.empty_like(valid) if max_norm is not None else None
    _lib.checked().smil_kp_triangulate(_ptr(kp), _ptr(vis), _ptr(view_mask), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), B, V, J, float(S),
                                       float(damping), float(max_norm or 0.0), ROT_DTYPES[kp.dtype], _ptr(points), _ptr(valid), _ptr(sane), _stream())
    return points, valid, sane


def kp_triangulate_backward(kp, vis, view_mask, R, T, fov, aspect, dpoints, S: float, damping: float, need=(True, True, True)):
    """``(d R, d T, d fov)`` from the gradient on the points (B,J,3)."""
    B, V, J = _kp_sizes(R, kp.shape[2])
    grads = tuple(torch.empty_like(t) if n else None for t, n in zip((R, T, fov), need))
    if any(need):
        _lib.checked().smil_kp_triangulate_backward(_ptr(kp), _ptr(vis), _ptr(view_mask), _ptr(R), _ptr(T), _ptr(fov), _ptr(aspect), _ptr(dpoints), B,
                                                    V, J, float(S), float(damping), ROT_DTYPES[kp.dtype], _ptr(_kp_f64(B, J, 6, device=kp.device)),
                                                    *(_ptr(g) for g in grads), _stream())
    return grads


# ---- rigid and similarity alignment of 3-D keypoint sets (csrc/align.hip) ----
# Conventions as above: contiguous tensors on one GPU, floats in one storage type of ROT_DTYPES, masks uint8 (or None), weights
# float64 (or None).  The status is an int32 device tensor: nothing here synchronises.
ALIGN_MODES = {"none": _lib.ALIGN_NONE, "rigid": _lib.ALIGN_RIGID, "similarity": _lib.ALIGN_SIMILARITY}


def align_forward(src: torch.Tensor, dst: torch.Tensor, weights, mask, with_scale: bool, min_gap: float, robust_iters: int,
                  robust_scale: float):
    """src, dst (B,J,3), weights (J) / (B,J) float64 or None, mask (B,J) uint8 or None -> ``(R (B,3,3), t (B,3), s (B), status (B) int32,
    gap (B), rms (B), w_final (B,J) float64, saved (B, ALIGN_SAVED) float64)``: smil_align_forward."""
    B, J = int(src.shape[0]), int(src.shape[1])
    new = lambda *shape, dtype=src.dtype: torch.empty(*shape, dtype=dtype, device=src.device)  # noqa: E731
    R, t, s, gap, rms = new(B, 3, 3), new(B, 3), new(B), new(B), new(B)
    status = new(B, dtype=torch.int32)
    w_final, saved = new(B, J, dtype=torch.float64), new(B, _lib.ALIGN_SAVED, dtype=torch.float64)
    _lib.checked().smil_align_forward(_ptr(src), _ptr(dst), _ptr(weights), int(weights is not None and weights.dim() == 2), _ptr(mask), B, J,
                                      int(bool(with_scale)), float(min_gap), int(robust_iters), float(robust_scale), ROT_DTYPES[src.dtype], _ptr(R),
                                      _ptr(t), _ptr(s), _ptr(status), _ptr(gap), _ptr(rms), _ptr(w_final), _ptr(saved), _stream())
    return R, t, s, status, gap, rms, w_final, saved


def align_backward(src, dst, w_final, saved, status, gR, gt, gs, with_scale: bool, need=(True, True)):
    """``(d src, d dst)``, each (B,J,3) or None where it is not needed, from the upstream gR, gt, gs (any None: zero)."""
    B, J = int(src.shape[0]), int(src.shape[1])
    dsrc = torch.empty_like(src) if need[0] else None
    ddst = torch.empty_like(dst) if need[1] else None
    if any(need):
        _lib.checked().smil_align_backward(_ptr(src), _ptr(dst), _ptr(w_final), _ptr(saved), _ptr(status), _ptr(gR), _ptr(gt), _ptr(gs), B, J,
                                           int(bool(with_scale)), ROT_DTYPES[src.dtype], _ptr(dsrc), _ptr(ddst), _stream())
    return dsrc, ddst


def align_errors(pred, target, mask, mode: int, sentinel: bool, scale: float, min_gap: float):
    """pred, target (B,J,3) -> ``(dist (B,J), valid (B,J) uint8, status (B) int32)``: smil_align_errors."""
    B, J = int(pred.shape[0]), int(pred.shape[1])
    dist = torch.empty(B, J, dtype=pred.dtype, device=pred.device)
    valid = torch.empty(B, J, dtype=torch.uint8, device=pred.device)
    status = torch.empty(B, dtype=torch.int32, device=pred.device)
    _lib.checked().smil_align_errors(_ptr(pred), _ptr(target), _ptr(mask), B, J, int(mode), int(bool(sentinel)), float(scale), float(min_gap),
                                     ROT_DTYPES[pred.dtype], _ptr(dist), _ptr(valid), _ptr(status), _stream())
    return dist, valid, status


# ---- mesh-free joint kinematics and the fused 3-D keypoint evaluation (csrc/joints.hip; tables: joints.py) ----
class DeviceJointTables:
    """``joints.JointTables`` resident on one GPU (``SmilJointTables``), with the workspace the sums over frames use: ONE zeroed
    buffer, grown when a call needs more, used by the calls on these tables in stream order (every call leaves its counter at zero)."""

    def __init__(self, jt, device):
        self.device = require_gpu(device)
        self.host = jt
        self.J, self.nB, self.P, self.static_joints = jt.J, jt.nB, jt.P, bool(jt.static_joints)
        s = _lib.JointTables()
        s.J, s.nB, s.P, s.max_depth, s.static_joints = jt.J, jt.nB, jt.P, jt.max_depth, int(jt.static_joints)
        self._keep = {}
        for name, dtype in (("parents", np.int32), ("depth", np.int32), ("child_ptr", np.int32), ("child", np.int32), ("J0", np.float64),
                            ("JB", np.float64), ("pair_ptr", np.int32), ("pair_bone", np.int32), ("M0", np.float64), ("MB", np.float64),
                            ("bpair_ptr", np.int32), ("bpair_joint", np.int32), ("bpair_index", np.int32), ("rowsum", np.float64)):
            a = np.ascontiguousarray(getattr(jt, name), dtype)
            if a.size:
                self._keep[name] = torch.from_numpy(a.copy()).to(self.device)
                setattr(s, name, self._keep[name].data_ptr())
        self.struct = s
        self._ws: Optional[torch.Tensor] = None

    def workspace(self, nbytes: int) -> Optional[torch.Tensor]:
        if nbytes == 0:
            return None
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws


def _joints_inputs(jt: DeviceJointTables, beta, theta, trans, logscale, btrans, theta_mask, fl: Dict) -> _lib.JointsInputs:
    """beta (B,nB_used) or (nB_used,) [shared]; theta (B,J,3); logscale / btrans (B,J,3) or (J,3) [shared] or None; trans (B,3) or None;
    ``fl``: trans_after_joints, propagate_scaling, allow_limb_scaling.  Shapes are checked here: a kernel never reads past a buffer."""
    B, J = int(theta.shape[0]), jt.J
    if tuple(theta.shape) != (B, J, 3):
        raise ValueError(f"theta must be (B,{J},3), got {tuple(theta.shape)}")
    if beta.dim() not in (1, 2) or (beta.dim() == 2 and beta.shape[0] != B) or beta.shape[-1] > jt.nB:
        raise ValueError(f"beta must be (B,nB_used) or (nB_used,) with B={B}, nB_used <= {jt.nB}; got {tuple(beta.shape)}")
    i = _lib.JointsInputs()
    i.B, i.shared_beta, i.nB_used = B, int(beta.dim() == 1), int(beta.shape[-1])
    i.beta, i.theta = _ptr(beta) if beta.numel() else None, _ptr(theta)
    for name, t in (("logscale", logscale), ("btrans", btrans)):
        if t is not None and tuple(t.shape) not in ((B, J, 3), (J, 3)):
            raise ValueError(f"{name} must be (B,{J},3) or ({J},3) with B={B}, got {tuple(t.shape)}")
        setattr(i, name, _ptr(t))
        setattr(i, name + "_shared", int(t is not None and t.dim() == 2))
    if trans is not None and tuple(trans.shape) != (B, 3):
        raise ValueError(f"trans must be (B,3) with B={B}, got {tuple(trans.shape)}")
    if theta_mask is not None and tuple(theta_mask.shape) != (J, 3):
        raise ValueError(f"theta_mask must be ({J},3), got {tuple(theta_mask.shape)}")
    i.trans, i.theta_mask = _ptr(trans), _ptr(theta_mask)
    i.trans_after_joints, i.propagate_scaling = int(fl.get("trans_after_joints", True)), int(fl.get("propagate_scaling", False))
    i.allow_limb_scaling = int(fl.get("allow_limb_scaling", True))
    for t in (beta, theta, trans, logscale, btrans, theta_mask):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != jt.device):
            raise ValueError("the joints kernels take contiguous float32 tensors on the tables' device")
    return i


def joints_forward(jt: DeviceJointTables, beta, theta, trans=None, logscale=None, btrans=None, theta_mask=None, want_new_J=True, **fl):
    """``(joints (B,J,3), new_J (B,J,3) or None)``: smil_joints_forward."""
    i = _joints_inputs(jt, beta, theta, trans, logscale, btrans, theta_mask, fl)
    joints = torch.empty(i.B, jt.J, 3, dtype=torch.float32, device=jt.device)
    new_J = torch.empty_like(joints) if want_new_J else None
    _lib.checked().smil_joints_forward(ctypes.byref(jt.struct), ctypes.byref(i), _ptr(joints), _ptr(new_J), _stream())
    return joints, new_J


def joints_backward(jt: DeviceJointTables, d_joints, beta, theta, trans=None, logscale=None, btrans=None, theta_mask=None,
                    need=("d_beta", "d_theta", "d_trans", "d_logscale", "d_btrans"), **fl) -> Dict[str, torch.Tensor]:
    """The gradients named in ``need`` (shapes of the inputs; a shared table's gradient is the sum over frames): smil_joints_backward."""
    i = _joints_inputs(jt, beta, theta, trans, logscale, btrans, theta_mask, fl)
    B, J = i.B, jt.J
    if tuple(d_joints.shape) != (B, J, 3) or d_joints.dtype != torch.float32 or not d_joints.is_contiguous():
        raise ValueError(f"d_joints must be a contiguous float32 ({B},{J},3) tensor")
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=jt.device)  # noqa: E731
    out = {}
    if "d_beta" in need and i.nB_used > 0:
        out["d_beta"] = new(*beta.shape)
    if "d_theta" in need:
        out["d_theta"] = new(B, J, 3)
    if "d_trans" in need:
        out["d_trans"] = new(B, 3)
    if "d_logscale" in need:
        out["d_logscale"] = new(*(logscale.shape if logscale is not None else (B, J, 3)))
    if "d_btrans" in need:
        out["d_btrans"] = new(*(btrans.shape if btrans is not None else (B, J, 3)))
    g = _lib.JointsGrads()
    g.d_joints = _ptr(d_joints)
    for k, v in out.items():
        setattr(g, k, _ptr(v))
    lib = _lib.checked()
    ws = jt.workspace(int(lib.smil_joints_backward_workspace_bytes(ctypes.byref(jt.struct), ctypes.byref(i), ctypes.byref(g))))
    g.workspace = _ptr(ws)
    lib.smil_joints_backward(ctypes.byref(jt.struct), ctypes.byref(i), ctypes.byref(g), _stream())
    return out


def kp3d_fit_eval(cfg: _lib.FitConfig, jt: DeviceJointTables, w_k3d: float, robust_scale: float, canon, target, visibility, joint_weights,
                  beta, theta, trans, logscale, btrans, theta_mask, objs, d_pose, d_trans, d_betas=None, d_logscale=None, d_btrans=None,
                  joints_out=None, **fl) -> None:
    """smil_kp3d_fit_eval: canon (Jc) int32 or None, target (N,Jc,3) float32, visibility (N,Jc) uint8 or None, joint_weights (Jc)
    float64 or None; objs[9] is added to, the gradient tensors are overwritten with the RAW gradients."""
    fl = dict(fl, trans_after_joints=True)
    i = _joints_inputs(jt, beta, theta, trans, logscale, btrans, theta_mask, fl)
    N, Jc = i.B, int(target.shape[1])
    if tuple(target.shape) != (N, Jc, 3) or target.dtype != torch.float32 or not target.is_contiguous():
        raise ValueError(f"target must be a contiguous float32 ({N},Jc,3) tensor, got {tuple(target.shape)} {target.dtype}")
    if canon is not None and (canon.dtype != torch.int32 or tuple(canon.shape) != (Jc,)):
        raise ValueError(f"canon must be int32 ({Jc},)")
    if visibility is not None and (visibility.dtype != torch.uint8 or tuple(visibility.shape) != (N, Jc) or not visibility.is_contiguous()):
        raise ValueError(f"visibility must be a contiguous uint8 ({N},{Jc}) tensor")
    if joint_weights is not None and (joint_weights.dtype != torch.float64 or tuple(joint_weights.shape) != (Jc,)):
        raise ValueError(f"joint_weights must be float64 ({Jc},)")
    lib = _lib.checked()
    ws = jt.workspace(int(lib.smil_kp3d_fit_eval_workspace_bytes(ctypes.byref(jt.struct), ctypes.byref(i), int(d_betas is not None),
                                                                 int(d_logscale is not None), int(d_btrans is not None))))
    lib.smil_kp3d_fit_eval(ctypes.byref(cfg), float(w_k3d), float(robust_scale), ctypes.byref(jt.struct), ctypes.byref(i), Jc, _ptr(canon),
                           _ptr(target), _ptr(visibility), _ptr(joint_weights), _ptr(objs), _ptr(d_pose), _ptr(d_trans), _ptr(d_betas),
                           _ptr(d_logscale), _ptr(d_btrans), _ptr(joints_out), _ptr(ws), _stream())


def kp2d_fit_eval(cfg: _lib.FitConfig, jt: DeviceJointTables, cams: CameraSet, w_k2d: float, robust_scale_px: float, canon, target2d,
                  visibility2d, confidence, joint_weights, beta, theta, trans, logscale, btrans, theta_mask, objs, d_pose=None, d_trans=None,
                  d_betas=None, d_logscale=None, d_btrans=None, joints_out=None, yx_out=None, w_k3d: float = 0.0, robust_scale: float = 0.0,
                  target3d=None, visibility3d=None, **fl) -> None:
    """smil_kp2d_fit_eval: ``cams`` a ``CameraSet`` of ``views`` views on S x S images (tables of 1, views or N*views rows); target2d
    (N,Nv,Jc,2) float32 in (y,x), visibility2d (N,Nv,Jc) uint8 or None, confidence (N,Nv,Jc) float32 or None, joint_weights (Jc)
    float64 or None, the optional 3-D term's target3d (N,Jc,3) / visibility3d (N,Jc) as in ``kp3d_fit_eval``.  objs[0] (and objs[9]) are
    added to, the gradient tensors are overwritten with the RAW gradients, yx_out (N,Nv,Jc,2) with the projections."""
    fl = dict(fl, trans_after_joints=True)
    i = _joints_inputs(jt, beta, theta, trans, logscale, btrans, theta_mask, fl)
    N, Nv = i.B, int(cams.views)
    if target2d.dim() != 4:
        raise ValueError(f"target2d must be (N,Nv,Jc,2), got {tuple(target2d.shape)}")
    Jc = int(target2d.shape[2])
    dev = jt.device

    def want(name, t, shape, dtype):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {dtype} {shape} tensor on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")

    want("target2d", target2d, (N, Nv, Jc, 2), torch.float32)
    want("visibility2d", visibility2d, (N, Nv, Jc), torch.uint8)
    want("confidence", confidence, (N, Nv, Jc), torch.float32)
    want("canon", canon, (Jc,), torch.int32)
    want("joint_weights", joint_weights, (Jc,), torch.float64)
    want("target3d", target3d, (N, Jc, 3), torch.float32)
    want("visibility3d", visibility3d, (N, Jc), torch.uint8)
    want("yx_out", yx_out, (N, Nv, Jc, 2), torch.float32)
    want("joints_out", joints_out, (N, jt.J, 3), torch.float32)
    if canon is None and Jc > jt.J:
        raise ValueError(f"Jc={Jc} above J={jt.J} without a canon list")
    cam = cams.struct(N * Nv)
    lib = _lib.checked()
    ws = jt.workspace(int(lib.smil_kp2d_fit_eval_workspace_bytes(ctypes.byref(jt.struct), ctypes.byref(i), ctypes.byref(cam),
                                                                 int(d_betas is not None), int(d_logscale is not None),
                                                                 int(d_btrans is not None))))
    lib.smil_kp2d_fit_eval(ctypes.byref(cfg), float(w_k2d), float(robust_scale_px), ctypes.byref(jt.struct), ctypes.byref(i), ctypes.byref(cam), Jc,
                           _ptr(canon), _ptr(target2d), _ptr(visibility2d), _ptr(confidence), _ptr(joint_weights), float(w_k3d), float(robust_scale),
                           _ptr(target3d), _ptr(visibility3d), _ptr(objs), _ptr(d_pose), _ptr(d_trans), _ptr(d_betas), _ptr(d_logscale),
                           _ptr(d_btrans), _ptr(joints_out), _ptr(yx_out), _ptr(ws), _stream())


def adam_step_multi_bc64(items, beta1=0.5, beta2=0.999, eps=1e-8):
    """``adam_step_multi`` through smil_adam_step_multi_bc64: the bias corrections formed in double, as torch.optim.Adam forms them."""
    _adam_multi("smil_adam_step_multi_bc64", items, beta1, beta2, eps)


# ---- visual hull (csrc/visual_hull.hip) -----------------------------------------------------------------------------------------
class HullGridSpec:
    """The grid of a visual hull (``SmilHullGrid``): ``N`` frames of ``grid = (Gx, Gy, Gz)`` voxels, x fastest; ``origin`` (1 or N, 3) the
    grid's corner and ``voxel_size`` (1 or N) the edge of a voxel, both HOST float64 (the library validates them on the host and uploads
    them itself)."""

    def __init__(self, N: int, grid, origin, voxel_size):
        if len(tuple(grid)) != 3:
            raise ValueError(f"grid must be (Gx, Gy, Gz), got {grid}")
        self.N = int(N)
        self.grid = tuple(int(g) for g in grid)
        host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x  # noqa: E731  (a Python float stays float64)
        self.origin = np.ascontiguousarray(np.asarray(host(origin), np.float64).reshape(-1, 3))
        self.voxel_size = np.ascontiguousarray(np.asarray(host(voxel_size), np.float64).reshape(-1))
        s = self.struct = _lib.HullGrid()
        s.N, (s.Gx, s.Gy, s.Gz) = self.N, self.grid
        s.origin, s.n_origin = self.origin.ctypes.data, self.origin.shape[0]
        s.voxel_size, s.n_voxel_size = self.voxel_size.ctypes.data, self.voxel_size.shape[0]

    @property
    def voxels(self) -> int:
        return self.grid[0] * self.grid[1] * self.grid[2]

    def shape(self):
        return (self.N, self.grid[2], self.grid[1], self.grid[0])


def _hull_masks(masks: torch.Tensor, N: int, views: int) -> torch.Tensor:
    if not isinstance(masks, torch.Tensor) or masks.dim() != 4 or masks.dtype not in (torch.uint8, torch.bool, torch.float32):
        raise ValueError("masks must be a uint8, bool or float32 tensor (N, Nv, H, W)")
    if masks.shape[0] != N or masks.shape[1] != views:
        raise ValueError(f"masks must be ({N},{views},H,W), got {tuple(masks.shape)}")
    masks = masks.contiguous()
    return masks.view(torch.uint8) if masks.dtype == torch.bool else masks


def hull_carve(spec: HullGridSpec, masks: torch.Tensor, cams: CameraSet, min_views: int, max_misses: int, outside_carves: bool = False,
               threshold: float = 0.0, want_counts: bool = False):
    """smil_hull_carve: masks (N,Nv,H,W) uint8, bool or float32 -> ``(occ, fg, seen)``, each (N,Gz,Gy,Gx) uint8 (fg, seen None unless
    ``want_counts``)."""
    dev = require_gpu(masks.device)
    N, Nv = spec.N, int(cams.views)
    masks = _hull_masks(masks, N, Nv)
    H, W = int(masks.shape[2]), int(masks.shape[3])
    lib = _lib.checked()
    cam = cams.struct(N * Nv)
    occ = torch.empty(spec.shape(), dtype=torch.uint8, device=dev)
    fg = torch.empty_like(occ) if want_counts else None
    seen = torch.empty_like(occ) if want_counts else None
    ws = _workspace(max(1, lib.smil_hull_carve_workspace_bytes(ctypes.byref(spec.struct))), dev)
    lib.smil_hull_carve(ctypes.byref(spec.struct), _ptr(masks), int(masks.dtype == torch.float32), H, W, float(threshold), ctypes.byref(cam),
                        int(min_views), int(max_misses), int(bool(outside_carves)), _ptr(occ), _ptr(fg), _ptr(seen), _ptr(ws), _stream())
    return occ, fg, seen


def hull_query(points: torch.Tensor, masks: torch.Tensor, cams: CameraSet, outside_carves: bool = False, threshold: float = 0.0):
    """smil_hull_query: points (N,P,3) float32 -> ``(fg, seen)`` (N,P) uint8."""
    dev = require_gpu(masks.device)
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points must be (N,P,3), got {tuple(points.shape)}")
    N, P, Nv = int(points.shape[0]), int(points.shape[1]), int(cams.views)
    points = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    masks = _hull_masks(masks, N, Nv)
    cam = cams.struct(N * Nv)
    fg = torch.empty(N, P, dtype=torch.uint8, device=dev)
    seen = torch.empty_like(fg)
    _lib.checked().smil_hull_query(_ptr(points), N, P, _ptr(masks), int(masks.dtype == torch.float32), int(masks.shape[2]), int(masks.shape[3]),
                                   float(threshold), ctypes.byref(cam), int(bool(outside_carves)), _ptr(fg), _ptr(seen), _stream())
    return fg, seen


def _hull_occ(spec: HullGridSpec, occ: torch.Tensor) -> torch.Tensor:
    if tuple(occ.shape) != spec.shape() or occ.dtype != torch.uint8:
        raise ValueError(f"occ must be a uint8 {spec.shape()} tensor, got {tuple(occ.shape)} {occ.dtype}")
    require_gpu(occ.device)
    return occ.contiguous()


def hull_stats(spec: HullGridSpec, occ: torch.Tensor) -> torch.Tensor:
    """smil_hull_stats: (N,16) int64 - count, the sums of i, j, k, of i^2, j^2, k^2, ij, ik, jk, the minima and the maxima of i, j, k over
    the occupied voxels."""
    occ = _hull_occ(spec, occ)
    stats = torch.empty(spec.N, _lib.HULL_STATS, dtype=torch.int64, device=occ.device)
    _lib.checked().smil_hull_stats(ctypes.byref(spec.struct), _ptr(occ), _ptr(stats), _stream())
    return stats


def hull_surface(spec: HullGridSpec, occ: torch.Tensor, want_index: bool = False):
    """smil_hull_surface_count / _write: ``(points (total,3) float32, index (total,) int64 or None, offsets (N+1,) int64)``.  The host
    waits ONCE, for ``offsets[N]``, to size the outputs."""
    occ = _hull_occ(spec, occ)
    dev = occ.device
    lib = _lib.checked()
    ws = _workspace(max(1, lib.smil_hull_surface_workspace_bytes(ctypes.byref(spec.struct))), dev)
    offsets = torch.empty(spec.N + 1, dtype=torch.int64, device=dev)
    lib.smil_hull_surface_count(ctypes.byref(spec.struct), _ptr(occ), _ptr(offsets), _ptr(ws), _stream())
    total = int(offsets[-1].item())
    points = torch.empty(total, 3, dtype=torch.float32, device=dev)
    index = torch.empty(total, dtype=torch.int64, device=dev) if want_index else None
    if total:
        lib.smil_hull_surface_write(ctypes.byref(spec.struct), _ptr(occ), _ptr(ws), _ptr(points), _ptr(index), _stream())
    return points, index, offsets


# ---- hull meshes (csrc/hull_mesh.hip) --------------------------------------------------------------------------------------------
def hull_mesh(spec: HullGridSpec, occ: torch.Tensor, weights=(), want_normals: bool = True):
    """smil_hull_mesh_count / _write: ``(verts (Vt,3) float32, normals (Vt,3) float32 or None, faces (Ft,3) int64 frame-local, vert_offsets
    (N+1,) int64, face_offsets (N+1,) int64)``.  ``weights``: the relaxation schedule, host float64.  The host waits ONCE, for the two
    totals, to size the outputs; nothing is launched for the write when both are 0."""
    occ = _hull_occ(spec, occ)
    dev = occ.device
    w = np.ascontiguousarray(np.asarray(tuple(weights), np.float64).reshape(-1))
    lib = _lib.checked()
    grid = ctypes.byref(spec.struct)
    ws = _workspace(max(1, lib.smil_hull_mesh_workspace_bytes(grid)), dev)
    offsets = torch.empty(2, spec.N + 1, dtype=torch.int64, device=dev)
    lib.smil_hull_mesh_count(grid, _ptr(occ), _ptr(offsets[0]), _ptr(offsets[1]), _ptr(ws), _stream())
    n_verts, n_faces = (int(t) for t in offsets[:, -1].tolist())
    verts = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(n_verts, 3, dtype=torch.float32, device=dev) if want_normals else None
    faces = torch.empty(n_faces, 3, dtype=torch.int64, device=dev)
    # (both totals 0: the call validates its arguments and launches nothing)
    scratch = _workspace(max(1, lib.smil_hull_mesh_scratch_bytes(n_verts, len(w))), dev)
    lib.smil_hull_mesh_write(grid, _ptr(occ), _ptr(ws), _ptr(scratch), n_verts, n_faces, w.ctypes.data if len(w) else None, len(w), _ptr(verts),
                             _ptr(normals), _ptr(faces), _stream())
    return verts, normals, faces, offsets[0], offsets[1]


# ---- distance fields (csrc/distance_field.hip) ----------------------------------------------------------------------------------
def hull_edt(spec: HullGridSpec, occ: torch.Tensor, invert: bool = False, border: bool = False) -> torch.Tensor:
    """smil_hull_edt: occ (N,Gz,Gy,Gx) uint8 -> d2 (N,Gz,Gy,Gx) int32, the squared voxel distance of every voxel to the nearest one with
    ``occ != 0`` (``invert``: ``== 0``; ``border``: the one-voxel layer around the grid counts too); ``_lib.EDT_NONE`` where there is none."""
    occ = _hull_occ(spec, occ)
    lib = _lib.checked()
    d2 = torch.empty(spec.shape(), dtype=torch.int32, device=occ.device)
    ws = _workspace(max(1, lib.smil_hull_edt_workspace_bytes(ctypes.byref(spec.struct))), occ.device)
    lib.smil_hull_edt(ctypes.byref(spec.struct), _ptr(occ), int(bool(invert)), int(bool(border)), _ptr(d2), _ptr(ws), _stream())
    return d2


def _field_grid(spec: HullGridSpec, d2: torch.Tensor, name: str) -> torch.Tensor:
    if tuple(d2.shape) != spec.shape() or d2.dtype != torch.int32:
        raise ValueError(f"{name} must be an int32 {spec.shape()} tensor, got {tuple(d2.shape)} {d2.dtype}")
    require_gpu(d2.device)
    return d2.contiguous()


def field_sample(spec: HullGridSpec, d2_out: torch.Tensor, d2_in: Optional[torch.Tensor], points: torch.Tensor, want_grad: bool = True):
    """smil_field_sample: points (N,P,3), or (N,P,2) ``(y, x)`` on a grid with Gz = 1 -> ``(value (N,P), grad (N,P,dim) or None)`` float32."""
    d2_out = _field_grid(spec, d2_out, "d2_out")
    d2_in = None if d2_in is None else _field_grid(spec, d2_in, "d2_in")
    dev = d2_out.device
    if points.dim() != 3 or points.shape[0] != spec.N or points.shape[2] not in (2, 3):
        raise ValueError(f"points must be ({spec.N},P,2 or 3), got {tuple(points.shape)}")
    P, dim = int(points.shape[1]), int(points.shape[2])
    points = _f32(points, dev)
    lib = _lib.checked()
    value = torch.empty(spec.N, P, dtype=torch.float32, device=dev)
    grad = torch.empty(spec.N, P, dim, dtype=torch.float32, device=dev) if want_grad else None
    if P == 0:  # (an empty tensor has no address to pass)
        return value, grad
    ws = _workspace(max(1, lib.smil_hull_carve_workspace_bytes(ctypes.byref(spec.struct))), dev)
    lib.smil_field_sample(ctypes.byref(spec.struct), _ptr(d2_out), _ptr(d2_in), _ptr(points), dim, P, _ptr(value), _ptr(grad), _ptr(ws), _stream())
    return value, grad
