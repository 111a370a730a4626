"""Multi-view visual hulls from silhouette masks (voxel carving): 3-D evidence for a silhouette-only sequence.

A voxel belongs to the hull if its CENTRE projects onto foreground in the views that see it.  ``carve`` tests every voxel of a regular
grid per frame in one HIP kernel (csrc/visual_hull.hip, one byte per voxel out; nothing of size voxels x views is ever stored);
``VisualHull`` turns the occupancy into what the 3-D side of the library takes - exact index statistics (count, centroid, covariance,
bounds), the packed surface voxels, a fixed-size surface sample for ``fit3d.chamfer_distance`` / ``pointnet2``, and the tight bounds for a
second, finer carve; ``VisualHull.extract_mesh`` the watertight triangle mesh with vertex normals (csrc/hull_mesh.hip) that ``fit3d``,
``mesh3d`` and ``sdf`` are written against.  ``query_points`` runs the same test at arbitrary points ("does this triangulated keypoint lie inside every outline").

Conventions (include/smilfit.h, "Visual hull"): the camera arithmetic is that of ``KeypointFitter2D`` (float64 on the float32 tables,
``(y, x)`` pixels of an ``image_size`` x ``image_size`` screen; with ``cameras.opencv_to_pinhole_camera(R, t, K, S)`` and ``image_size=S`` the
screen coordinates are source pixels for ANY ``S``, so masks of full, non-square camera frames need no crop).  ``cameras`` is a
``cameras.FoVCameras`` or the dict ``KeypointFitter2D`` takes; every table holds 1, ``views`` or ``N * views`` rows.  Pixel ``(r, c)`` of a mask
covers ``[r, r+1) x [c, c+1)``; a view sees a point iff it lies more than the near plane (0.001) in front of the camera and inside the
``H x W`` mask; a seen point is foreground iff the mask value is ``> threshold`` (a float NaN is background).

Limits.  A voxel is tested at its centre only: keep ``voxel_size`` at or below a pixel's footprint (``z / (image_size/2 * k11)``) or thin
limbs fall between the centres.  One wrong mask or a calibration error carves for good: for noisy masks or calibration, dilate the masks
first (``torch.nn.functional.max_pool2d(masks.float(), 2 r + 1, 1, r)``) or raise ``max_misses``.  There are no gradients through the
carve itself; ``VisualHull.distance_field`` gives the differentiable term that pulls points towards (or into) a carved hull.  At most 64
views.  ``origin`` and ``voxel_size`` are host values (a device tensor is copied back, which waits for the device).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, engine
from .fit_keypoints2d import _camera_set

MAX_VIEWS = _lib.HULL_MAX_VIEWS


class HullStats(NamedTuple):
    count: torch.Tensor       # (N,) int64: occupied voxels
    centroid: torch.Tensor    # (N,3) float64, world units; NaN for an empty frame
    covariance: torch.Tensor  # (N,3,3) float64, world units squared (population covariance of the occupied centres); NaN if empty
    index_min: torch.Tensor   # (N,3) int64 (i, j, k); the grid's extent for an empty frame
    index_max: torch.Tensor   # (N,3) int64; -1 for an empty frame


def _check_masks(masks) -> Tuple[int, int]:
    if not isinstance(masks, torch.Tensor) or masks.dim() != 4:
        raise ValueError("masks must be a tensor (N, Nv, H, W)")
    N, Nv = int(masks.shape[0]), int(masks.shape[1])
    if not 1 <= Nv <= MAX_VIEWS:
        raise _lib.SmilError(f"visual hull: views={Nv} outside 1..{MAX_VIEWS}")
    return N, Nv


def _image_size(image_size) -> int:
    if int(image_size) != image_size or int(image_size) < 1:
        raise ValueError(f"image_size must be a positive integer, got {image_size}")
    return int(image_size)


def gibson_steps(n: int) -> Tuple[float, ...]:
    """``n`` steps of weight 0.5: Gibson's constrained SurfaceNets relaxation (smooths, and shrinks)."""
    return (0.5,) * int(n)


def taubin_steps(n: int) -> Tuple[float, ...]:
    """``n`` pairs (0.5, -0.53): Taubin's lambda | mu smoothing, which keeps the volume."""
    return (0.5, -0.53) * int(n)


class HullMesh:
    """The triangle meshes of a hull's frames, packed: ``verts (Vt,3)`` float32 (world units), ``normals (Vt,3)`` float32 unit vertex
    normals pointing out of the hull (None unless asked for), ``faces (Ft,3)`` int64 indices into the frame's OWN vertices,
    ``vert_offsets`` / ``face_offsets (N+1,)`` int64: frame ``n`` owns ``verts[vert_offsets[n]:vert_offsets[n+1]]`` and
    ``faces[face_offsets[n]:face_offsets[n+1]]``.  Every frame's mesh is closed and consistently oriented (each directed edge is met by
    its reverse).  There is no gradient through the extraction."""

    def __init__(self, verts, normals, faces, vert_offsets, face_offsets):
        self.verts, self.normals, self.faces = verts, normals, faces
        self.vert_offsets, self.face_offsets = vert_offsets, face_offsets
        self._bounds = None

    def __len__(self) -> int:
        return int(self.vert_offsets.shape[0]) - 1

    def _host_offsets(self):
        if self._bounds is None:  # (one copy for both tables)
            self._bounds = torch.stack([self.vert_offsets, self.face_offsets]).tolist()
        return self._bounds

    def _split(self, packed, which: int) -> List[torch.Tensor]:
        off = self._host_offsets()[which]
        return [packed[off[n]:off[n + 1]] for n in range(len(self))]

    def verts_list(self) -> List[torch.Tensor]:
        return self._split(self.verts, 0)

    def normals_list(self) -> List[torch.Tensor]:
        if self.normals is None:
            raise ValueError("this mesh was extracted with return_normals=False")
        return self._split(self.normals, 0)

    def faces_list(self) -> List[torch.Tensor]:
        return self._split(self.faces, 1)

    def to_meshes(self, keep: Optional[Sequence[int]] = None):
        """``mesh3d.Meshes`` of the frames (``keep``: of these frames, in this order), built from lists.  A frame without a hull has no
        mesh: it raises a ValueError that names the frame - select the others with ``keep``."""
        from .mesh3d import Meshes

        frames = list(range(len(self))) if keep is None else [int(n) for n in keep]
        verts, faces = self.verts_list(), self.faces_list()
        for n in frames:
            if not -len(self) <= n < len(self):
                raise ValueError(f"to_meshes: frame {n} outside the hull's {len(self)} frames")
            if verts[n].shape[0] == 0:
                raise ValueError(f"to_meshes: frame {n} has an empty hull and no mesh; pass keep= to select the other frames")
        return Meshes(verts=[verts[n] for n in frames], faces=[faces[n] for n in frames])

    def volume(self) -> torch.Tensor:
        """(N,) float64: the signed volume every frame's mesh encloses (the divergence theorem's sum over its triangles, in float64 tensor
        operations on the device); positive, since the faces point outwards; 0 for a frame without a hull."""
        N = len(self)
        out = torch.zeros(N, dtype=torch.float64, device=self.verts.device)
        if self.faces.shape[0] == 0:
            return out
        rows = torch.arange(self.faces.shape[0], device=self.faces.device)
        frame = torch.searchsorted(self.face_offsets[1:].contiguous(), rows, right=True)
        tri = self.verts.to(torch.float64)[self.faces + self.vert_offsets[frame][:, None]]
        six = (tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum(-1)
        return out.index_add_(0, frame, six) / 6.0


class VisualHull:
    """The result of ``carve``: ``occupancy (N,Gz,Gy,Gx)`` uint8, ``fg`` / ``seen`` (the per-voxel view counts, or None), and the grid
    (``origin (1 or N,3)``, ``voxel_size (1 or N)`` float64 on the host, ``grid = (Gx, Gy, Gz)``).  Voxel ``(i, j, k)`` has the centre
    ``origin + ((i, j, k) + 0.5) * voxel_size`` and the linear index ``i + Gx (j + Gy k)``."""

    def __init__(self, occupancy, fg, seen, spec: engine.HullGridSpec):
        self.occupancy, self.fg, self.seen = occupancy, fg, seen
        self._spec = spec
        self.grid = spec.grid
        self.origin = torch.from_numpy(spec.origin.copy())
        self.voxel_size = torch.from_numpy(spec.voxel_size.copy())

    def _raw_stats(self) -> torch.Tensor:
        return engine.hull_stats(self._spec, self.occupancy)

    def stats(self) -> HullStats:
        """Count, centroid, covariance and index bounds of the occupied voxels of every frame.  The kernel returns exact int64 sums of the
        voxel indices; the float64 moments are formed from them with tensor operations on the device (no synchronisation).  A frame
        with no occupied voxel returns NaN rows (and ``index_min = grid``, ``index_max = -1``); it does not raise."""
        s = self._raw_stats()
        dev = s.device
        n = s[:, 0].to(torch.float64)
        mean = s[:, 1:4].to(torch.float64) / n[:, None]  # (0 / 0 = NaN for an empty frame)
        second = torch.empty(s.shape[0], 3, 3, dtype=torch.float64, device=dev)
        for (a, b), col in (((0, 0), 4), ((1, 1), 5), ((2, 2), 6), ((0, 1), 7), ((0, 2), 8), ((1, 2), 9)):
            second[:, a, b] = second[:, b, a] = s[:, col].to(torch.float64) / n
        origin = self.origin.to(dev).expand(s.shape[0], 3)
        voxel = self.voxel_size.to(dev).expand(s.shape[0])
        cov = (second - mean[:, :, None] * mean[:, None, :]) * (voxel * voxel)[:, None, None]
        return HullStats(s[:, 0], origin + (mean + 0.5) * voxel[:, None], cov, s[:, 10:13], s[:, 13:16])

    def surface_points(self, return_index: bool = False):
        """``(points (total,3) float32, offsets (N+1,) int64)``: the centres of the surface voxels - occupied, with an unoccupied
        6-neighbour, the grid's border counting as unoccupied - packed frame after frame in ascending linear voxel index; frame ``n``
        owns rows ``offsets[n]:offsets[n+1]``.  ``return_index``: ``(points, index (total,) int64, offsets)`` with the linear voxel indices.
        This call SYNCHRONISES the host once, to read the total and size the output."""
        points, index, offsets = engine.hull_surface(self._spec, self.occupancy, want_index=return_index)
        return (points, index, offsets) if return_index else (points, offsets)

    def sample_surface(self, num_samples: int, seed: int = 0) -> torch.Tensor:
        """(N,S,3) float32: ``num_samples`` surface points per frame, drawn uniformly with replacement by ``engine.sample_vertices`` from the
        packed surface - the fixed-size cloud ``fit3d.chamfer_distance`` and ``pointnet2`` take.  A frame with an empty hull gives zeros, as
        that function documents.  One host synchronisation (``surface_points``)."""
        points, offsets = self.surface_points()
        N = self._spec.N
        if points.shape[0] == 0:
            return torch.zeros(N, int(num_samples), 3, dtype=torch.float32, device=points.device)
        if points.shape[0] >= 2**31:
            raise _lib.SmilError(f"sample_surface: {points.shape[0]} surface voxels exceed the sampler's 32-bit offsets")
        values = torch.zeros(points.shape[0], dtype=torch.float32, device=points.device)
        out, _, _ = engine.sample_vertices(points, values, offsets.to(torch.int32), N, int(num_samples), seed)
        return out

    def extract_mesh(self, relax_steps: Sequence[float] = (), return_normals: bool = True) -> HullMesh:
        """The hull's boundary as a ``HullMesh``: surface nets on the lattice of voxel centres (include/smilfit.h, "Hull meshes").  One
        vertex per cube of 8 neighbouring voxel centres that are not all of one kind, one quad (two triangles) per pair of 6-neighbours
        of which exactly one is occupied - the grid's border counting as unoccupied, so a hull that touches the grid is closed there.
        ``relax_steps``: a schedule of relaxation weights, each step moving every vertex towards the mean of its neighbours and back
        into its own cube - ``gibson_steps(n)`` smooths and shrinks, ``taubin_steps(n)`` smooths and keeps the volume; the default ``()``
        leaves the vertices at the mean of their cube's edge crossings (which cuts corners: a single voxel becomes a cube of a third
        of its edge).  Voxels that touch only along an edge share that edge four-fold: the mesh stays closed and oriented, but is not a
        manifold there.  ``return_normals``: area-weighted unit vertex normals.  No gradient.  This call SYNCHRONISES the host once,
        to read the two totals and size the outputs."""
        return HullMesh(*engine.hull_mesh(self._spec, self.occupancy, relax_steps, want_normals=return_normals))

    def distance_transform(self, inside: bool = False, border: bool = False) -> torch.Tensor:
        """(N,Gz,Gy,Gx) int32: the exact squared Euclidean distance, in voxels, from every voxel to the nearest occupied one (``inside``:
        to the nearest unoccupied one).  ``border``: the one-voxel layer around the grid counts as a target too (for ``inside`` this is
        ``surface_points``' rule that the border is unoccupied, and keeps the inside distance of a full grid finite).  Centre to centre:
        a target voxel reads 0.  A frame without a target reads ``_lib.EDT_NONE`` (2^31 - 1) everywhere.  Integer arithmetic: the result
        is the definition's, bit for bit."""
        return engine.hull_edt(self._spec, self.occupancy, invert=inside, border=border)

    def distance_field(self, signed: bool = False) -> "HullDistanceField":
        """The hull's distance field for ``HullDistanceField.sample`` / ``containment_loss``: ``distance_transform()``, and for ``signed``
        also ``distance_transform(inside=True, border=True)``; the signed field is negative inside the hull and positive outside."""
        return HullDistanceField(self._spec, self.distance_transform(), self.distance_transform(inside=True, border=True) if signed else None)

    def tight_bounds(self, margin_voxels: int = 1):
        """``(origin (N,3), voxel_size (N,))`` float64 of a grid of the same ``grid`` extent around every frame's occupied index range
        ``index_min .. index_max`` widened by ``margin_voxels`` coarse voxels on every side: the second pass of a coarse-to-fine carve
        (``carve(..., origin=origin, voxel_size=voxel_size, grid=hull.grid)``).  The new voxels are cubes sized by the axis that needs the
        largest ones, the box is centred on the occupied range.  A frame with an empty hull keeps its grid."""
        s = self._raw_stats()
        dev = s.device
        N = s.shape[0]
        origin = self.origin.to(dev).expand(N, 3)
        voxel = self.voxel_size.to(dev).expand(N)
        G = torch.tensor(self.grid, dtype=torch.float64, device=dev)
        lo = (s[:, 10:13] - int(margin_voxels)).to(torch.float64)
        hi = (s[:, 13:16] + 1 + int(margin_voxels)).to(torch.float64)
        new_voxel = ((hi - lo) / G).amax(dim=1) * voxel
        centre = origin + 0.5 * (lo + hi) * voxel[:, None]
        new_origin = centre - 0.5 * G * new_voxel[:, None]
        empty = (s[:, 0] == 0)
        return torch.where(empty[:, None], origin, new_origin), torch.where(empty, voxel, new_voxel)


class _FieldSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, spec, d2_out, d2_in):
        want = points.requires_grad
        value, grad = engine.field_sample(spec, d2_out, d2_in, points, want_grad=want)
        ctx.save_for_backward(grad) if want else ctx.save_for_backward()
        ctx.want = want
        return value

    @staticmethod
    def backward(ctx, g):
        if not ctx.want:
            return None, None, None, None
        (grad,) = ctx.saved_tensors
        return g[..., None] * grad, None, None, None


class HullDistanceField:
    """A distance field on the grid of a hull: ``d2_out (N,Gz,Gy,Gx)`` int32 (squared voxel distances to the hull), ``d2_in`` (to its
    complement; None for an unsigned field), and the grid (``origin``, ``voxel_size``, ``grid`` as on ``VisualHull``).

    The field at a point (include/smilfit.h, "Distance fields"): per axis ``u = (p - origin) / voxel_size - 0.5`` is the continuous index
    (cell centres on the integers); the cell values ``voxel_size * (sqrt(d2_out) - sqrt(d2_in))`` are interpolated trilinearly between the
    centres, and outside the box of cell centres the distance to that box is added, so the field is continuous and a point outside the
    grid is pulled back to it.  A frame without a hull reads 0 everywhere (no pull), a point with a NaN or infinite coordinate reads 0
    with gradient 0 (the keypoint fitters' "not there").  The transform is centre to centre: a point inside an occupied voxel but off its
    centre reads a small positive interpolated value near the surface.  At an integer ``u`` the slope is that of the cell to the right
    (to the left at the last cell)."""

    def __init__(self, spec: engine.HullGridSpec, d2_out: torch.Tensor, d2_in=None):
        self._spec, self.d2_out, self.d2_in = spec, d2_out, d2_in
        self.grid = spec.grid
        self.origin = torch.from_numpy(spec.origin.copy())
        self.voxel_size = torch.from_numpy(spec.voxel_size.copy())

    @property
    def signed(self) -> bool:
        return self.d2_in is not None

    def sample(self, points: torch.Tensor) -> torch.Tensor:
        """(N,P) float32: the field at ``points (N,P,3)`` (world units), differentiable in the points (one gather kernel forward, which also
        stores the gradient; the backward multiplies).  There is no gradient to the field."""
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"points must be a tensor (N,P,3), got {tuple(getattr(points, 'shape', ()))}")
        return _FieldSampleFn.apply(points, self._spec, self.d2_out, self.d2_in)

    def containment_loss(self, points: torch.Tensor, weights=None) -> torch.Tensor:
        """The mean of ``sample(points) ** 2`` (with ``weights (N,P)``: the weighted mean, ``sum(w s^2) / sum(w)``): zero when every point
        lies on a hull voxel's centre (unsigned field), growing with the squared distance to the hull."""
        s2 = self.sample(points) ** 2
        if weights is None:
            return s2.mean()
        w = torch.as_tensor(weights, dtype=s2.dtype, device=s2.device)
        return (w * s2).sum() / w.sum()


def carve(masks, cameras, *, image_size: int, origin, voxel_size, grid, min_views: int = 2, max_misses: int = 0,
          outside_carves: bool = False, threshold: float = 0.0, return_counts: bool = False) -> VisualHull:
    """Carve a ``grid = (Gx, Gy, Gz)`` of cubic voxels per frame from ``masks (N,Nv,H,W)`` (uint8, bool or float32, on the GPU).

    ``origin`` ((3,) or (N,3)) is the grid's corner, ``voxel_size`` (a number or (N,)) the edge of a voxel.  A voxel is occupied iff
    ``seen >= min_views and seen - fg <= max_misses``, with ``seen`` the views that see its centre and ``fg`` those in which it is foreground.
    ``outside_carves``: a view in front of which the centre lies but outside the image counts as seen and as a miss (by default such a view
    does not vote).  ``return_counts``: keep the per-voxel ``fg`` and ``seen`` (two more bytes per voxel)."""
    N, Nv = _check_masks(masks)
    dev = engine.require_gpu(masks.device)
    cams = _camera_set(cameras, Nv, N, _image_size(image_size), dev)
    spec = engine.HullGridSpec(N, grid, origin, voxel_size)
    occ, fg, seen = engine.hull_carve(spec, masks, cams, min_views, max_misses, outside_carves, threshold, want_counts=return_counts)
    return VisualHull(occ, fg, seen, spec)


def query_points(points, masks, cameras, *, image_size: int, threshold: float = 0.0, outside_carves: bool = False):
    """``(fg, seen)`` (N,P) uint8: in how many views each of ``points (N,P,3)`` is foreground, and how many see it (``outside_carves``: are in
    front of it) - the test of ``carve`` at arbitrary points.  A point lies inside every outline iff ``fg == seen == Nv``."""
    N, Nv = _check_masks(masks)
    dev = engine.require_gpu(masks.device)
    cams = _camera_set(cameras, Nv, N, _image_size(image_size), dev)
    return engine.hull_query(torch.as_tensor(points), masks, cams, outside_carves, threshold)
