"""Drop-ins for the reference's 3-D registration program (fitter_3d/trainer.py, fitter_3d/optimise.py) on the HIP path.

``fitter_3d/trainer.py`` runs unchanged once its pytorch3d imports read::

    from smilify_amd.fit3d import sample_points_from_meshes, chamfer_distance, mesh_edge_loss, \\
        mesh_laplacian_smoothing, mesh_normal_consistency
    from smilify_amd.fit3d import SDF_distance, sample_points_from_meshes_and_SDF  # fitter_3d.utils
    from smilify_amd.mesh3d import Meshes

and this module carries its ``SMAL3DFitter`` / ``SMALParamGroup`` / ``Stage`` / ``StageManager`` as well, with the SMAL half on the
existing LBS kernels and every loss on the kernels of ``csrc/mesh3d.hip``.  Each loss is a ``torch.autograd.Function`` whose forward
computes the loss and its gradient in one launch sequence; backward scales that gradient.

Deviations: sampling draws from a Philox counter-based generator keyed by a 64-bit seed taken from torch's
default CPU generator, so ``torch.manual_seed`` makes runs reproducible but the points differ from pytorch3d's (torch.multinomial /
torch.rand / torch.randint streams).  The SDF term (``SDF_distance``, ``knn_points``, ``sample_points_from_meshes_and_SDF``)
orders neighbours by (squared distance, index) and supports 1 <= K <= 64, K <= the number of candidates and clouds of at least two
points.  The per-vertex diameter values it loads are computed by ``smilify_amd.sdf``.  Out of scope and raising: the SDF heat
maps, loss / mesh plots, normals / lengths / norm=1 in chamfer_distance, knn_points and SDF_distance, the cot / cotcurv Laplacians.

Run as ``python -m smilify_amd.fit3d --model MODEL.npz --mesh_dir DIR [--yaml_src CFG.yaml] [--use_sdf --sdf_dir DIR]``
(fitter_3d/optimise.py).
"""
from __future__ import annotations

import argparse
import os
import pickle
from collections import namedtuple
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
    (pytorch3d.ops.sample_points_from_meshes, trainer.py:376).  ``return_normals``: ``(points, normals)``, the normals (N, num_samples, 3)
    being the unit normals of the faces the points were drawn on (pytorch3d's rule), gathered from the sampler's face indices with
    tensor operations.  No gradient: raises if the vertices require one."""
    if return_textures:
        raise NotImplementedError("sample_points_from_meshes: return_textures is not supported")
    vl = meshes.verts_list()
    if any(v.requires_grad for v in vl):
        raise NotImplementedError("sample_points_from_meshes: the HIP sampler has no gradient; detach the vertices first")
    pts, face = sample_points_with_faces(meshes, num_samples)
    if not return_normals:
        return pts
    first = torch.tensor([0] + meshes.num_faces_per_mesh()[:-1], dtype=torch.int64).cumsum(0).to(face.device)
    tri = _gpu_f32(meshes.verts_packed())[meshes.faces_packed().to(face.device)[face.to(torch.int64) + first[:, None]]]  # (N,S,3,3)
    n = torch.linalg.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
    return pts, n / n.norm(dim=-1, keepdim=True).clamp(min=torch.finfo(torch.float32).tiny)


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


# ---- the SDF-guided term (fitter_3d/utils.py:973-1394) --------------------------------------------------------------------------
_KNN = namedtuple("KNN", "dists idx knn")


def _check_clouds(what: str, x, y) -> None:
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dim() == 3 and y.dim() == 3 and x.shape[2] == 3
            and y.shape[2] == 3 and x.shape[0] == y.shape[0]):
        raise ValueError(f"{what}: x (N,P1,3) and y (N,P2,3) tensors")


class _KnnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, K):
        a, b = _gpu_f32(p1), _gpu_f32(p2)
        dists, idx, _, _, _ = engine.knn(a, b, K)
        idx = idx.long()
        ctx.save_for_backward(a, b, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    def backward(ctx, g, _):
        # d dists[n,i,k] = 2 (p1_i - p2_j): gathered for p1, summed per candidate in float64 for p2 (not on the Stage's path, which
        # takes the fused term's gradient from the kernel)
        a, b, idx = ctx.saved_tensors
        N, P1, K = idx.shape
        flat = idx.reshape(N, P1 * K, 1).expand(-1, -1, 3)
        e = (a[:, :, None, :] - torch.gather(b, 1, flat).reshape(N, P1, K, 3)).double() * (2.0 * g.double())[..., None]
        d2 = torch.zeros(b.shape, dtype=torch.float64, device=b.device).scatter_add_(1, flat, -e.reshape(N, P1 * K, 3))
        return e.sum(2).float(), d2.float(), None


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True):
    """pytorch3d.ops.knn_points for (N,P1,3) / (N,P2,3) tensors without lengths: (dists (N,P1,K) squared, idx (N,P1,K) int64, knn
    None), every row ascending by (distance, index)."""
    if lengths1 is not None or lengths2 is not None:
        raise NotImplementedError("knn_points: lengths are not supported")
    if norm != 2:
        raise NotImplementedError("knn_points: only norm=2")
    if return_nn:
        raise NotImplementedError("knn_points: return_nn is not supported (gather p2 at idx)")
    _check_clouds("knn_points", p1, p2)
    dists, idx = _KnnFn.apply(p1, p2, int(K))
    return _KNN(dists, idx, None)


class _SdfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, x_sdf, y_sdf, K, single_directional, point_sum, batch_sum):
        want = x.requires_grad or y.requires_grad
        loss, dx, dy, _, _ = engine.sdf_distance(_gpu_f32(x), _gpu_f32(y), _gpu_f32(x_sdf), _gpu_f32(y_sdf), K, single_directional,
                                                 point_sum, batch_sum, want_grad=want)
        ctx.save_for_backward(dx, dy) if want else ctx.save_for_backward()
        ctx.want = want
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.want:
            return (None,) * 8
        dx, dy = ctx.saved_tensors
        return (dx * g, dy * g) + (None,) * 6


def SDF_distance(x, y, x_sdf, y_sdf, k: int, batch_reduction="mean", point_reduction="mean", norm: int = 2,
                 single_directional: bool = False, visualize: bool = False, output_dir: str = "sdf_visualization",
                 title: str = "sdf_loss_contribution", mesh_names=None):
    """fitter_3d.utils.SDF_distance: with the per-cloud z-scores of the values and the k nearest candidates (d_ik, j_ik) of every
    query, sum_k softmax_k(-|z_q[i] - z_c[j_ik]| / 0.1) d_ik, reduced over points and meshes, both directions added.  The values
    carry no gradient (the reference's do, but they are data in its Stage)."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    if norm != 2:
        raise NotImplementedError("SDF_distance: only norm=2")
    if visualize:
        raise NotImplementedError("SDF_distance: the heat-map visualisation is not supported")
    if point_reduction not in ("mean", "sum") or batch_reduction not in ("mean", "sum"):
        raise NotImplementedError("SDF_distance: point_reduction / batch_reduction must be 'mean' or 'sum'")
    _check_clouds("SDF_distance", x, y)
    if not (isinstance(x_sdf, torch.Tensor) and isinstance(y_sdf, torch.Tensor) and x_sdf.shape == x.shape[:2]
            and y_sdf.shape == y.shape[:2]):
        raise ValueError("SDF_distance: x_sdf (N,P1) and y_sdf (N,P2) must match the clouds")
    if k < 1:
        raise ValueError("k must be at least 1")
    return _SdfFn.apply(x, y, x_sdf, y_sdf, int(k), bool(single_directional), point_reduction == "sum", batch_reduction == "sum")


def _pack_sdf_values(meshes: Meshes, sdf_values):
    """The three forms of ``sdf_values`` (a (V,) tensor shared by all meshes, an (N,V) tensor, a list of N (V_n,) tensors) as one
    packed float32 tensor on the meshes' device, with the meshes' vertex offsets: (values, vert_off int32, n_verts, max_verts)."""
    nv = meshes.num_verts_per_mesh()
    N, dev = len(meshes), meshes.device
    if isinstance(sdf_values, (list, tuple)):
        if len(sdf_values) != N:
            raise ValueError(f"Number of SDF value tensors ({len(sdf_values)}) must match number of meshes ({N})")
        rows = [torch.as_tensor(v).reshape(-1) for v in sdf_values]
    elif isinstance(sdf_values, torch.Tensor):
        if sdf_values.dim() == 1:
            if any(n != nv[0] for n in nv):
                raise ValueError("When providing a single 1D tensor of SDF values, all meshes must have the same number of vertices")
            rows = [sdf_values] * N
        elif sdf_values.dim() == 2 and sdf_values.shape[0] == N:
            rows = list(sdf_values.unbind(0))
        else:
            raise ValueError(f"sdf_values of shape {tuple(sdf_values.shape)} for {N} meshes: expected (V,) or ({N}, V)")
    else:
        raise TypeError("sdf_values must be either a list of tensors or a single tensor")
    for n, (r, v) in enumerate(zip(rows, nv)):
        if int(r.shape[0]) != v:
            raise ValueError(f"Number of SDF values ({int(r.shape[0])}) must match number of vertices ({v}) of mesh {n}")
    values = torch.cat([r.detach().to(device=dev, dtype=torch.float32) for r in rows]).contiguous()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)).to(dev)
    return values, off, int(sum(nv)), int(max(nv))


class _SampleVertsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_packed, packed, N, S, seed):
        values, off, n_verts, max_verts = packed
        pts, val, idx = engine.sample_vertices(_gpu_f32(verts_packed), values, off, N, S, seed)
        ctx.save_for_backward(idx, off)
        ctx.sizes = (n_verts, max_verts)
        ctx.mark_non_differentiable(val, idx)
        return pts, val, idx

    @staticmethod
    def backward(ctx, g, _v, _i):
        idx, off = ctx.saved_tensors
        return engine.sample_vertices_backward(g.to(torch.float32).contiguous(), idx, off, *ctx.sizes), None, None, None, None


def sample_vertices_with_index(meshes: Meshes, sdf_values, num_samples: int, seed: Optional[int] = None, _packed=None):
    """(points (N,S,3) with gradient to the vertices, values (N,S), vertex index within its mesh (N,S) int32).  ``seed`` None: a
    63-bit value from torch's default generator."""
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
    packed = _packed if _packed is not None else _pack_sdf_values(meshes, sdf_values)
    engine.require_gpu(meshes.device)
    return _SampleVertsFn.apply(meshes.verts_packed(), packed, len(meshes), int(num_samples), int(seed))


def sample_points_from_meshes_and_SDF(meshes: Meshes, sdf_values, num_samples: int = 10000):
    """fitter_3d.utils.sample_points_from_meshes_and_SDF: ``num_samples`` vertices of every mesh, uniform with replacement, and their
    values: (samples (N,S,3), sdf_samples (N,S)).  Values whose length is not the mesh's vertex count raise ValueError."""
    pts, val, _ = sample_vertices_with_index(meshes, sdf_values, num_samples)
    return pts, val


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


# ---- exact point <-> mesh distances (csrc/point_mesh.hip; an extension, pytorch3d's loss.point_mesh_face_distance) -----------------
class _PointMeshFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_packed, points, mt, lengths, by_face, bvh=None):
        v, p = _gpu_f32(verts_packed), _gpu_f32(points)
        dist2, idx, _ = _search(v, mt, p, lengths, by_face, bvh)
        ctx.save_for_backward(v, p, idx)
        ctx.call = (mt, lengths, by_face)
        idx = idx.long()
        ctx.mark_non_differentiable(idx)
        return dist2, idx

    @staticmethod
    def backward(ctx, g, _):
        v, p, idx = ctx.saved_tensors
        mt, lengths, by_face = ctx.call
        d_points, d_verts = engine.point_mesh_backward(v, mt, p, lengths, idx, g.to(torch.float32).contiguous(), by_face)
        return d_verts, d_points, None, None, None, None


def _search(v, mt, p, lengths, by_face: bool, bvh):
    """The forward search: the brute force, or - points -> faces only - the hierarchy ``bvh`` (``mesh3d.MeshBVH``), which records the
    same faces, so that the backward is the same call on the same records."""
    if bvh is None:
        return engine.point_mesh_distance(v, mt, p, lengths, by_face)
    return bvh.query(p, lengths, verts=v)[:3]


def _point_mesh(meshes: Meshes, points, lengths, by_face: bool, bvh=None):
    if not (isinstance(points, torch.Tensor) and points.dim() == 3 and points.shape[2] == 3 and points.shape[0] == len(meshes)):
        raise ValueError(f"points ({len(meshes)},P,3) for {len(meshes)} meshes")
    engine.require_gpu(meshes.device)
    if bvh is not None:
        bvh._check(meshes)
    return _PointMeshFn.apply(meshes.verts_packed(), points, meshes.face_tables(), lengths, by_face, bvh)


def point_face_distance(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, bvh=None):
    """(dist2 (N,P), face (N,P) int64): for every point of ``points`` (N,P,3) the squared Euclidean distance to the nearest closed
    triangle of its mesh and that face's index within the mesh.  Differentiable in ``points`` and in the meshes' vertices (through
    ``offset_verts`` too); the indices carry no gradient.  Points at or beyond ``lengths`` (N), non-finite points and meshes without a
    usable face give ``inf`` and -1 and receive no gradient.  Exact: a brute-force search; with ``bvh``, a ``mesh3d.MeshBVH`` built
    or refitted on these meshes' vertices, the same records and hence the same values and gradients, bit for bit, through the
    hierarchy."""
    return _point_mesh(meshes, points, lengths, False, bvh)


def face_point_distance(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None):
    """(dist2 (F_total), point (F_total) int64): for every face of the packed meshes the squared distance to the nearest point of its
    mesh's cloud and that point's index within the cloud (-1 and ``inf`` for a cloud without a finite point).  Differentiable as
    ``point_face_distance``."""
    return _point_mesh(meshes, points, lengths, True)


def point_mesh_face_distance(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pytorch3d.loss.point_mesh_face_distance's normalisation on the exact distances: the mean over each cloud's points of the
    point -> face term plus the mean over each mesh's faces of the face -> point term, averaged over the batch.  Entries without a
    partner (index -1) add 0.  The true distance to the closed triangle; pytorch3d's min_triangle_area rule is not reproduced."""
    N, P = len(meshes), int(points.shape[1])
    d_pf, face = point_face_distance(meshes, points, lengths)
    d_fp, point = face_point_distance(meshes, points, lengths)
    mt = meshes.face_tables()
    n_pts = torch.full((N,), float(P), device=d_pf.device) if lengths is None else lengths.to(d_pf.device, torch.float32).clamp(min=1.0)
    n_faces = (mt.face_off[1:] - mt.face_off[:-1]).to(torch.float32).clamp(min=1.0)
    mesh_of_face = torch.repeat_interleave(torch.arange(N, device=d_pf.device), (mt.face_off[1:] - mt.face_off[:-1]).long(),
                                           output_size=mt.n_faces)
    per_cloud = torch.where(face >= 0, d_pf, torch.zeros_like(d_pf)).sum(1) / n_pts
    per_mesh = torch.zeros(N, device=d_pf.device, dtype=d_fp.dtype).index_add(0, mesh_of_face,
                                                                               torch.where(point >= 0, d_fp, torch.zeros_like(d_fp)))
    return (per_cloud.sum() + (per_mesh / n_faces).sum()) / N


def _masked_mean(dist2: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return torch.where(idx >= 0, dist2, torch.zeros_like(dist2)).mean()


# ---- signed distances and containment (the winding numbers of csrc/point_mesh.hip decide the side) -------------------------------
def _inside(meshes: Meshes, points: torch.Tensor, lengths, oriented: bool) -> torch.Tensor:
    """(N,P) bool from the winding numbers (``mesh3d.contains``); a constant of every backward."""
    w = engine.point_mesh_winding(_gpu_f32(meshes.verts_packed()), meshes.face_tables(), _gpu_f32(points), lengths)
    return (w if oriented else w.abs()) > 0.5


class _SignedDistanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_packed, points, mt, lengths, inside, bvh=None):
        v, p = _gpu_f32(verts_packed), _gpu_f32(points)
        dist2, idx, _ = _search(v, mt, p, lengths, False, bvh)
        sign = torch.where(inside, -torch.ones_like(dist2), torch.ones_like(dist2))
        ctx.save_for_backward(v, p, idx, dist2, sign)
        ctx.call = (mt, lengths)
        idx = idx.long()
        ctx.mark_non_differentiable(idx)
        return sign * dist2.sqrt(), idx

    @staticmethod
    def backward(ctx, g, _):
        v, p, idx, dist2, sign = ctx.saved_tensors
        mt, lengths = ctx.call
        live = (dist2 > 0) & (idx >= 0)  # d sqrt(d2) = d d2 / (2 sqrt(d2)); on the surface and without a face: exactly 0
        up = torch.where(live, g.to(torch.float32) * sign / (2.0 * torch.where(live, dist2, torch.ones_like(dist2)).sqrt()),
                         torch.zeros_like(dist2))
        d_points, d_verts = engine.point_mesh_backward(v, mt, p, lengths, idx, up.contiguous(), False)
        return d_verts, d_points, None, None, None, None


def _check_cloud_batch(meshes: Meshes, points) -> None:
    if not (isinstance(points, torch.Tensor) and points.dim() == 3 and points.shape[2] == 3 and points.shape[0] == len(meshes)):
        raise ValueError(f"points ({len(meshes)},P,3) for {len(meshes)} meshes")
    engine.require_gpu(meshes.device)


def point_mesh_signed_distance(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, oriented: bool = True, *,
                               bvh=None):
    """(sdist (N,P), face (N,P) int64): the Euclidean distance of every point to the surface of its mesh, negative inside, and the
    nearest face.  Inside: the generalised winding number is > 0.5 (``oriented=False``: its magnitude, for scans with inward faces);
    see ``mesh3d.winding_number`` for what that means on open or self-intersecting meshes.  Differentiable in the points and in the
    meshes' vertices: the gradient of ``sign * sqrt(dist2)`` at the recorded face, the sign a constant; exactly 0 for a point on the
    surface (dist2 == 0) and where there is no face (+inf, -1).  ``bvh``: as in ``point_face_distance``, for the distance; the winding
    numbers stay the brute-force sum."""
    _check_cloud_batch(meshes, points)
    if bvh is not None:
        bvh._check(meshes)
    return _SignedDistanceFn.apply(meshes.verts_packed(), points, meshes.face_tables(), lengths, _inside(meshes, points, lengths, oriented),
                                   bvh)


def _one_sided_loss(meshes: Meshes, points, lengths, weights, oriented: bool, want_inside: bool, bvh=None) -> torch.Tensor:
    _check_cloud_batch(meshes, points)
    N, P = len(meshes), int(points.shape[1])
    dist2, face = point_face_distance(meshes, points, lengths, bvh=bvh)
    inside = _inside(meshes, points, lengths, oriented)
    counted = (face >= 0) & (inside if want_inside else ~inside)
    valid = torch.ones(N, P, dtype=torch.bool, device=dist2.device) if lengths is None else \
        torch.arange(P, device=dist2.device)[None] < lengths.to(dist2.device)[:, None]
    w = valid.to(dist2.dtype) if weights is None else torch.as_tensor(weights, dtype=dist2.dtype, device=dist2.device) * valid
    norm = w.sum(1)
    norm = torch.where(norm > 0, norm, torch.ones_like(norm))
    return ((w * torch.where(counted, dist2, torch.zeros_like(dist2))).sum(1) / norm).sum() / N  # (the masked side: upstream 0)


def containment_loss(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, weights=None, oriented: bool = True, *,
                     bvh=None):
    """Pulls points INTO their meshes: per cloud the mean over its valid points (``weights`` (N,P): the weighted mean, sum(w x) /
    sum(w)) of the squared distance to the surface where the point is outside and 0 where it is inside, averaged over the batch.  The
    mesh counterpart of ``HullDistanceField.containment_loss``, at the mesh's own resolution.  C1 at the surface (no square root);
    inside points, points without a face and points beyond ``lengths`` receive exactly no gradient.  ``bvh``: as in
    ``point_face_distance``."""
    return _one_sided_loss(meshes, points, lengths, weights, oriented, False, bvh)


def penetration_loss(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, weights=None, oriented: bool = True, *,
                     bvh=None):
    """Pushes points OUT of their meshes: ``containment_loss`` with the roles swapped - the squared distance to the surface where the
    point is inside, 0 where it is outside."""
    return _one_sided_loss(meshes, points, lengths, weights, oriented, True, bvh)


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
    iteration plus the mesh regularisers, and the SDF-guided term when ``w_sdf`` > 0 and both value sets are given).  An extension:
    ``loss_weights["w_surface"]`` > 0 (absent from ``default_weights``: off) adds ``comps["surface"]``, the mean exact squared distance
    of the iteration's target samples to the source surface plus that of the source vertices to the target surfaces;
    ``loss_weights["w_contain"]`` > 0 (absent as well) adds ``comps["contain"]``, ``containment_loss`` of the source vertices in the
    target meshes - meant for hull meshes as targets."""

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
        if visualize_sdf_loss:
            raise NotImplementedError("SDF loss visualisation is not supported")
        self.sdf_values, self.source_sdf_values = sdf_values, source_sdf_values
        self.sdf_vis_frequency = sdf_vis_frequency
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
        # the values, packed once for the sampler (the vertex counts are fixed for the stage): a wrong length raises here
        self._sdf_packed = None
        if sdf_values is not None and source_sdf_values is not None:
            self._sdf_packed = (_pack_sdf_values(self.src_mesh, source_sdf_values), _pack_sdf_values(target_meshes, sdf_values))

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
        if self.consider_loss("sdf") and self._sdf_packed is not None:  # trainer.py:399-433: 10000 vertices a side, K = 50
            src_pts, src_sdf, _ = sample_vertices_with_index(src_mesh, None, 10000, _packed=self._sdf_packed[0])
            tgt_pts, tgt_sdf, _ = sample_vertices_with_index(self.target_meshes, None, 10000, _packed=self._sdf_packed[1])
            comps["sdf"] = SDF_distance(src_pts, tgt_pts, src_sdf, tgt_sdf, k=50, batch_reduction="mean", point_reduction="mean",
                                        norm=2, single_directional=False)
            loss = loss + self.loss_weights["w_sdf"] * comps["sdf"]
        w_surface = self.loss_weights.get("w_surface", 0)
        if w_surface > 0:  # an extension: exact distances to the surfaces instead of chamfer between samples and vertices
            to_source = _masked_mean(*point_face_distance(src_mesh, target_verts))  # reaches the model through the barycentrics
            to_target = _masked_mean(*point_face_distance(self.target_meshes, src_mesh.verts_padded()))  # ... through the points
            comps["surface"] = to_source + to_target
            loss = loss + w_surface * comps["surface"]
        w_contain = self.loss_weights.get("w_contain", 0)
        if w_contain > 0:  # an extension: the source vertices must lie inside the targets (hull meshes: a posed model inside its hull)
            comps["contain"] = containment_loss(self.target_meshes, src_mesh.verts_padded())
            loss = loss + w_contain * comps["contain"]
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


def load_sdf_values(mesh_name: str, sdf_dir: str, device) -> Optional[torch.Tensor]:
    """The per-vertex values of one mesh: ``NAME_sdf.npz`` (array ``vertex_sdf``), else ``NAME_sdf.pkl`` (a dict with a
    ``vertex_sdf`` tensor, optimise.py:113-142); the name is tried as given and without a 4-character extension.  None: no file."""
    for name in (mesh_name, mesh_name[:-4]):
        npz, pkl = os.path.join(sdf_dir, f"{name}_sdf.npz"), os.path.join(sdf_dir, f"{name}_sdf.pkl")
        if os.path.exists(npz):
            with np.load(npz) as d:
                return torch.from_numpy(np.asarray(d["vertex_sdf"], np.float32).reshape(-1)).to(device)
        if os.path.exists(pkl):
            with open(pkl, "rb") as fh:
                data = pickle.load(fh)
            if "vertex_sdf" not in data:
                raise KeyError(f"vertex_sdf not found in {pkl}")
            return torch.as_tensor(data["vertex_sdf"], dtype=torch.float32).reshape(-1).to(device)
    return None


def check_and_load_sdf_values(mesh_names, sdf_dir: str, device):
    """optimise.py:145-171: the values of every mesh (None where there is no file), with the reference's warning."""
    out = [load_sdf_values(n, sdf_dir, device) for n in mesh_names]
    missing = [n for n, v in zip(mesh_names, out) if v is None]
    if missing:
        print(f"\nWarning: SDF values not found for {len(missing)} meshes:")
        for n in missing:
            print(f"  - {n}")
    return out


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
    p.add_argument("--use_sdf", action="store_true", help="add the SDF-guided term (needs --sdf_dir)")
    p.add_argument("--sdf_dir", type=str, default=None,
                   help="directory of NAME_sdf.npz / NAME_sdf.pkl files (vertex_sdf) for the source model and the target meshes")
    p.add_argument("--w_surface", type=float, default=0.0,
                   help="weight of the exact point-to-surface term of every stage (an extension; 0: off, nothing changes)")
    p.add_argument("--w_contain", type=float, default=0.0,
                   help="weight of the containment term of every stage: the model's vertices inside the target meshes, for hull meshes "
                        "as targets (an extension; 0: off, nothing changes)")
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
    source_sdf_values = None
    if getattr(args, "use_sdf", False):  # optimise.py:202-228: the source model's file is required
        if not args.sdf_dir:
            raise ValueError("--use_sdf needs --sdf_dir")
        model_file = args.model if args.model is not None else _config.current.SMAL_FILE
        source_name = os.path.splitext(os.path.basename(model_file))[0]
        source_sdf_values = load_sdf_values(source_name, args.sdf_dir, args.device)
        if source_sdf_values is None:
            raise FileNotFoundError(f"SDF file for source model not found at {os.path.join(args.sdf_dir, source_name + '_sdf.npz')} "
                                    "(or .pkl). Compute the values of the source model first "
                                    "(python -m smilify_amd.sdf MESH_DIR --model MODEL).")
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
        if source_sdf_values is not None:
            tv = check_and_load_sdf_values(names, args.sdf_dir, args.device)
            if all(v is not None for v in tv):  # (the reference hands over the list as it is and fails on a None inside)
                kw.update(sdf_values=tv, source_sdf_values=source_sdf_values)
        surface = {k: float(getattr(args, k)) for k in ("w_surface", "w_contain") if getattr(args, k, 0) > 0} or None
        if stage_options is not None:
            for stage_name, skw in stage_options.items():
                if surface is not None:  # under the stage's own weights
                    skw = dict(skw, loss_weights=dict(surface, **(skw.get("loss_weights") or {})))
                manager.add_stage(Stage(name=f"{stage_name}_batch_{b}" if n_batches > 1 else stage_name, **skw, **kw))
                if b == 0:
                    stage_names.append(stage_name)
        else:
            manager.add_stage(Stage(scheme=args.scheme, nits=args.nits, lr=args.lr, name=f"stage_batch_{b}" if n_batches > 1 else "stage",
                                    loss_weights=surface, **kw))
            if b == 0:
                stage_names.append("stage")
        manager.run()
    if n_batches > 1:
        combine_stage_results(args.results_dir, stage_names, n_batches)
    return stage_names


if __name__ == "__main__":
    main(build_parser().parse_args())
