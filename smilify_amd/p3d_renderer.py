"""Drop-in ``Renderer`` module: same constructor, attributes and ``forward`` contract as the reference's
``smal_fitter.p3d_renderer.Renderer`` (reference smal_fitter/p3d_renderer.py:21-152), without pytorch3d.

``forward(vertices, points, faces)`` returns ``(silhouettes (B,1,S,S), projected points (B,P,2) in (y,x) px)``.
Gradients flow to ``vertices``, ``points`` and ``cameras.fov``.  The colour (HardPhong) branch of the reference is opt-in:
``Renderer(S, device, colour=True)`` makes ``forward(..., render_texture=True)`` return ``(sil, proj, colour (B,3,S,S))`` as the
reference does; with the default ``colour=False`` that call raises, as it always has.  ``render_colour(vertices, faces)`` is always
available.  The colour image carries no gradient (the reference uses it under ``no_grad`` for visualisation only).
"""
from __future__ import annotations

import hashlib
import weakref
from typing import Optional

import numpy as np
import torch

from . import config as _config
from . import engine, model_io
from .cameras import FoVCameras, look_at_view_transform


class _MeshTopology:
    """Face table resident on the GPU for meshes that do not come from a SMAL model."""

    def __init__(self, faces: np.ndarray, V: int, device):
        J = 1
        t = model_io.SmilModelTables(
            name="topology", v_template=np.zeros((V, 3), np.float32), shapedirs=np.zeros((0, 3 * V), np.float32),
            faces=faces.astype(np.int32), parents=np.array([-1], np.int32), depth=np.zeros(1, np.int32),
            skin_idx=np.zeros((V, 4), np.int32), skin_w=np.concatenate([np.ones((V, 1), np.float32), np.zeros((V, 3), np.float32)], 1),
            jreg_rowptr=np.zeros(J + 1, np.int32), jreg_col=np.zeros(0, np.int32), jreg_val=np.zeros(0, np.float32),
            static_joints=True, J_static=np.zeros((1, 3), np.float32))
        self.dm = engine.DeviceModel(t, device)


class _RenderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dm, cams, S, rs, joints_only, vertices, points, fov):
        v = vertices.detach().float().contiguous()
        p = points.detach().float().contiguous()
        cams = engine.CameraSet(cams.R, cams.T, fov.detach().float().contiguous(), cams.aspect, cams.views, S, cams.principal)
        _, yx = engine.project(cams, p, want_ndc=False)
        ctx.dm, ctx.cams, ctx.S, ctx.rs, ctx.joints_only = dm, cams, S, rs, joints_only
        if joints_only:
            ctx.save_for_backward(v, p)
            return torch.zeros(0, device=v.device), yx
        ndc, _ = engine.project(cams, v, want_yx=False)
        sil = engine.silhouette_forward(dm, ndc, S, rs)
        ctx.save_for_backward(v, p, ndc)
        return sil[:, None], yx

    @staticmethod
    def backward(ctx, g_sil, g_yx):
        cams = ctx.cams
        if ctx.joints_only:
            v, p = ctx.saved_tensors
            ndc = None
        else:
            v, p, ndc = ctx.saved_tensors
        N = p.shape[0] * cams.views
        d_fov_img = torch.zeros(N, dtype=torch.float32, device=p.device)
        d_v = None
        if ndc is not None and g_sil is not None and ctx.needs_input_grad[5]:
            cd = engine.clip_depth_for(ctx.dm, N)  # depth gradients of edges cut at the clipping plane (empty unless the mesh reaches the camera)
            d_ndc = engine.silhouette_backward(ctx.dm, ndc, ctx.S, g_sil.reshape(N, ctx.S, ctx.S).contiguous().float(), ctx.rs, clip_depth=cd)
            d_v, _ = engine.project_backward(cams, v, d_ndc=d_ndc, d_fov_img=d_fov_img)
            engine.clip_depth_backward(cams, cd, d_v)
        d_p = None
        if g_yx is not None:
            d_p, _ = engine.project_backward(cams, p, d_yx=g_yx.contiguous().float(), d_fov_img=d_fov_img)
        d_fov = engine.fov_reduce(cams, d_fov_img) if ctx.needs_input_grad[7] else None
        return None, None, None, None, None, d_v, d_p, d_fov


class Renderer(torch.nn.Module):
    DEFAULT_ZNEAR = 0.001  # reference p3d_renderer.py:24-25
    DEFAULT_ZFAR = 1000.0

    def __init__(self, image_size, device, views: int = 1, colour: bool = False):
        super().__init__()
        self.image_size = int(image_size)
        self.device = engine.require_gpu(device)
        self.views = int(views)
        self.colour = bool(colour)
        mesh_color = _config.current.MESH_COLOR if _config.current is not None else [0, 172, 223]  # reference :29 (config.MESH_COLOR)
        self.mesh_color = torch.tensor(mesh_color, dtype=torch.float32, device=self.device)[None, None, :] / 255.0
        R, T = look_at_view_transform(2.7, 0, 0, device=self.device)  # reference :34
        self.cameras = FoVCameras(R, T, torch.tensor([60.0], device=self.device), None, self.DEFAULT_ZNEAR, self.DEFAULT_ZFAR)
        self.raster_settings = engine.raster_settings()
        self._topologies = {}
        self._bound_model: Optional[engine.DeviceModel] = None
        self._bound_faces_ok = {}

    def bind_model(self, dm: engine.DeviceModel) -> None:
        """Use the face table already resident with a SMAL model (skips the per-call topology lookup)."""
        self._bound_model = dm
        self._bound_faces_ok = {}

    def set_camera_parameters(self, R, T, fov, aspect_ratio=None, principal_point=None):
        """Same contract as reference p3d_renderer.py:72-125 (fov squeezed to 1-D, scalar aspect broadcast).  ``principal_point``
        (an extension): ``(k,2)`` or ``(2,)`` values ``(px, py)`` in NDC, k = 1, views or images - the cameras become pytorch3d's
        ``PerspectiveCameras``, ``x_ndc = K00 x / z + px`` (``cameras.opencv_to_pinhole_camera``).  A constant: no gradient."""
        dev = self.device
        R = R.to(device=dev, dtype=torch.float32).reshape(-1, 3, 3).contiguous()
        T = T.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        fov = fov.to(device=dev, dtype=torch.float32)
        if fov.dim() > 1:
            fov = fov.squeeze(-1)
        if fov.dim() == 0:
            fov = fov.unsqueeze(0)
        if aspect_ratio is not None:
            if not isinstance(aspect_ratio, torch.Tensor):
                aspect_ratio = torch.tensor(aspect_ratio, dtype=torch.float32, device=dev)
            aspect_ratio = aspect_ratio.to(device=dev, dtype=torch.float32).reshape(-1)
            if aspect_ratio.numel() == 1 and fov.numel() > 1:
                aspect_ratio = aspect_ratio.expand_as(fov).contiguous()
        self.cameras = FoVCameras(R, T, fov, aspect_ratio, self.DEFAULT_ZNEAR, self.DEFAULT_ZFAR, self._principal_table(principal_point))

    def _principal_table(self, principal_point) -> Optional[torch.Tensor]:
        if principal_point is None:
            return None
        if isinstance(principal_point, torch.Tensor) and principal_point.requires_grad:
            raise NotImplementedError("the principal point carries no gradient: pass a tensor that does not require one")
        pp = torch.as_tensor(principal_point).to(device=self.device, dtype=torch.float32)
        if pp.numel() == 0 or pp.numel() % 2 or (pp.dim() > 1 and pp.shape[-1] != 2):
            raise ValueError(f"principal_point must be (k,2) values (px, py), got shape {tuple(pp.shape)}")
        return pp.reshape(-1, 2).contiguous()

    def _device_model(self, faces: torch.Tensor, V: int) -> engine.DeviceModel:
        """Face table on the GPU for the mesh topology passed to ``forward`` (the reference rasterises whatever faces it is
        given).  The bound SMAL model's table is used only for that model's own ``faces`` tensor; other topologies are
        uploaded once and cached by CONTENT (a hash of the index bytes), never by a tensor address that may be recycled
        (a faces[0] view of an expanded batch is a fresh object per call and is compared by content each time)."""
        f = faces[0] if faces.dim() == 3 else faces
        # Verified once per (storage address, in-place version, shape, dtype) of the tensor the CALLER holds: the reference passes
        # an expanded (B,F,3) view of one (F,3) tensor on every call (fitter.py:286-288), whose faces[0] is a fresh view object each
        # time but always the same storage - later calls with it cost a dictionary lookup, no device compare and no host sync.
        # A weak reference to the tensor that owns the storage (the view's base) guards against an address recycled for other
        # indices: a dead owner is a miss.
        owner = faces._base if faces._base is not None else faces
        skey = (faces.untyped_storage().data_ptr(), faces.storage_offset(), faces._version, tuple(f.shape), faces.dtype, tuple(faces.stride()[-2:]))
        hit = self._bound_faces_ok.get(skey)
        if hit is not None and hit[0]() is owner:
            return hit[1]
        dm = self._bound_model
        if dm is not None and dm.V == V and dm.F == f.shape[0] and torch.equal(f.to(device=self.device, dtype=torch.int32), dm.faces_i32()):
            found = dm
        else:
            host = np.ascontiguousarray(f.detach().cpu().numpy().astype(np.int32))
            key = (hashlib.sha1(host.tobytes()).hexdigest(), tuple(host.shape), V)
            if key not in self._topologies:
                self._topologies[key] = _MeshTopology(host, V, self.device)
            found = self._topologies[key].dm
        if len(self._bound_faces_ok) > 64:
            self._bound_faces_ok.clear()
        self._bound_faces_ok[skey] = (weakref.ref(owner), found)
        return found

    def _camera_set(self) -> engine.CameraSet:
        cam = self.cameras
        return engine.CameraSet(cam.R.contiguous(), cam.T.contiguous(), cam.fov.detach().float().reshape(-1).contiguous(),
                                None if cam.aspect_ratio is None else cam.aspect_ratio.contiguous(), self.views, self.image_size,
                                self._principal())

    def _principal(self) -> Optional[torch.Tensor]:
        """``cameras.principal_point`` as the kernels take it (the holder is mutable: callers may have assigned any tensor)."""
        pp = getattr(self.cameras, "principal_point", None)
        if pp is None:
            return None
        if pp.requires_grad:
            raise NotImplementedError("the principal point carries no gradient: pass a tensor that does not require one")
        return pp.contiguous()

    def render_colour(self, vertices, faces) -> torch.Tensor:
        """The reference's colour branch (p3d_renderer.py:54-70,148-150: hard rasteriser, K = 1, + HardPhongShader, point light at
        (0, 0, 3), the mesh in ``mesh_color``): (B * views, 3, S, S) float32, background 1.0, image n = frame * views + view.  No
        gradient."""
        dm = self._device_model(faces, vertices.shape[1])
        with torch.no_grad():
            return engine.render_colour(dm, self._camera_set(), vertices.detach().float().contiguous(), self.mesh_color.reshape(3).tolist())

    def render_fragments(self, vertices, faces, want=engine.FRAGMENT_OUTPUTS) -> engine.Fragments:
        """What the hard rasteriser of the colour branch finds per pixel (p3d_renderer.py:54-70: blur 0, K = 1), as an
        ``engine.Fragments`` tuple over B * views images, image n = frame * views + view: ``pix_to_face`` (n,S,S) int32 face id of
        the mesh (-1: background), ``zbuf`` (n,S,S) view depth (-1), ``bary`` (n,S,S,3) perspective-correct barycentrics of the
        original face (-1) and ``dist`` (n,S,S) the distance from the camera centre to the surface point (+inf).  No gradient."""
        dm = self._device_model(faces, vertices.shape[1])
        with torch.no_grad():
            return engine.render_fragments(dm, self._camera_set(), vertices.detach().float().contiguous(), want=want)

    def render_depth(self, vertices, faces, kind: str = "z") -> torch.Tensor:
        """Depth map (B * views, S, S) float32 of the mesh: ``kind="z"`` the view depth (background -1, pytorch3d's ``zbuf``),
        ``kind="distance"`` the Euclidean distance from the camera centre (background +inf), the convention of a depth pass that
        ``visibility.refine_visibility_with_depth`` tests keypoints against.  No gradient."""
        if kind not in ("z", "distance"):
            raise ValueError(f"kind must be 'z' or 'distance', got {kind!r}")
        name = "zbuf" if kind == "z" else "dist"
        return getattr(self.render_fragments(vertices, faces, want=(name,)), name)

    def keypoint_visibility(self, vertices, points, faces, tolerance: float, neighborhood: int = 1, visibility=None) -> torch.Tensor:
        """Which of ``points`` (B,P,3) the mesh ``vertices`` (B,V,3) hides from each camera: (B * views, P) float32, 1 = visible (or
        whatever ``visibility`` (B * views, P) held coming in), 0 where the point lies more than ``tolerance`` behind the nearest
        surface seen within ``neighborhood`` pixels of its projection.  The test is the reference's depth refinement
        (Unreal2Pytorch3D.py:664-760) run against the mesh's own distance map instead of a rendered depth PNG; points that project
        outside the image, onto background, or that are not finite keep their visibility.

        ``tolerance`` is in world units.  Model joints lie INSIDE the skin, so every one of them is behind the surface it is seen
        through: the tolerance must exceed the depth of the joints under that surface, or interior joints are declared hidden - the
        reference's own note at :712-717 (there with one LSB of the 8-bit depth pass on top, which a float map does not have).
        No gradient."""
        cams = self._camera_set()
        S, views = self.image_size, self.views
        with torch.no_grad():
            pts = points.detach().float().contiguous()
            B, P = pts.shape[0], pts.shape[1]
            N = B * views
            dist_map = self.render_depth(vertices, faces, kind="distance")
            _, yx = engine.project(cams, pts, want_ndc=False)
            kp_norm = yx.double() / float(S)
            # the points' distances to each image's camera centre C = -T R^T, in float64
            img = torch.arange(N, device=pts.device)
            R = cams.R.double()[img % cams.R.shape[0]]
            T = cams.T.double()[img % cams.T.shape[0]]
            centre = -torch.einsum("nk,nqk->nq", T, R)
            kp_dist = (pts.double()[img // views] - centre[:, None]).norm(dim=-1)
            if visibility is None:
                vis = torch.ones(N, P, dtype=torch.float32, device=pts.device)
            else:
                vis = torch.as_tensor(visibility).to(device=pts.device, dtype=torch.float32).reshape(N, P)
            return engine.depth_visibility(dist_map, kp_norm.contiguous(), kp_dist.contiguous(), vis, tolerance, neighborhood)

    def forward(self, vertices, points, faces, render_texture=False, joints_only=False):
        if render_texture and not self.colour:
            raise NotImplementedError("colour output is opt-in: construct Renderer(image_size, device, colour=True) "
                                      "(SMALFitter: FitterConfig.RENDER_COLOUR = True), or call render_colour()")
        cam = self.cameras
        B = vertices.shape[0]
        views = self.views
        N = B * views
        pp = self._principal()
        cs = engine.CameraSet(cam.R.contiguous(), cam.T.contiguous(), cam.fov, None if cam.aspect_ratio is None else cam.aspect_ratio.contiguous(),
                              views, self.image_size, pp)
        for name, k in (("R", cam.R.shape[0]), ("T", cam.T.shape[0]), ("fov", cam.fov.numel())) + (() if pp is None else (("principal_point", pp.shape[0]),)):
            if k not in (1, views, N):
                raise ValueError(f"cameras.{name} has {k} entries for {N} images")
        dm = None if joints_only else self._device_model(faces, vertices.shape[1])
        sil, proj = _RenderFunction.apply(dm, cs, self.image_size, self.raster_settings, bool(joints_only), vertices, points, cam.fov)
        if joints_only:
            return None, proj
        if render_texture:
            return sil, proj, self.render_colour(vertices, faces)
        return sil, proj
