"""Mesh plumbing of the 3-D registration path: the subset of pytorch3d's ``Meshes`` / ``load_obj`` that the reference's
``fitter_3d`` uses (trainer.py:3-9,33-36,359-362,413-415; utils.py:301-358), without pytorch3d.

* ``load_obj(path)`` reads ``v`` and ``f`` records only; polygons are fan-triangulated; ``i``, ``i/j``, ``i//k``, ``i/j/k`` and
  negative (relative) indices are accepted.
* ``Meshes(verts=..., faces=...)`` holds a batch of meshes (lists or padded tensors) and caches the host-side tables its losses
  need: the regulariser ``Topology`` of a shared face array and the float64 cumulative-area table used by surface sampling.
* ``Topology(faces, V)`` builds, once per face array: unique edges ``(v0 < v1)``, normal-consistency pairs ``(v0, v1, a, b)``,
  the Laplacian neighbour CSR with ``1/deg`` and the vertex -> pair incidence CSR.
* ``closest_points(meshes, points)`` (an extension): for every point the exact closest point of its mesh's surface - squared
  distance, face, barycentrics - on the kernels of csrc/point_mesh.hip: the registration metric.
* ``winding_number`` / ``contains`` / ``signed_distance`` (an extension): on which side of its mesh's surface a point lies, by the
  generalised winding number (the same file's k_pm_winding).
* ``MeshBVH(meshes)`` (an extension): a face hierarchy built once for meshes that stay put (csrc/mesh_bvh.hip); ``closest_points(...,
  bvh=)`` and the distance half of ``signed_distance(..., bvh=)`` then give the brute force's bits without the scan over all faces.
"""
from __future__ import annotations

import hashlib
import os
from collections import namedtuple
from typing import List, Optional

import numpy as np
import torch

from . import engine


def load_obj(path: str):
    """(verts (V,3) float32, faces (F,3) int64) of an OBJ file: ``v`` and ``f`` records, polygons fanned from their first corner."""
    verts: List[List[float]] = []
    faces: List[List[int]] = []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                if len(idx) < 3:
                    raise ValueError(f"{path}: face with {len(idx)} corners: {line.strip()}")
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index out of range [0, {len(v)})")
    return torch.from_numpy(v), torch.from_numpy(f)


def load_meshes(mesh_dir=None, mesh_files=None, sorting=lambda arr: arr, n_meshes=None, frame_step=1, device="cuda:0"):
    """(mesh names, Meshes) of a directory / list of OBJ files, each centred on its vertex mean and divided by its largest absolute
    coordinate (reference fitter_3d/utils.py:301-358)."""
    if mesh_dir is not None and mesh_files is not None:
        raise ValueError("Cannot specify both mesh_dir and mesh_files")
    if mesh_dir is not None:
        obj_list = sorting([f for f in os.listdir(mesh_dir) if ".obj" in f])[::frame_step]
        if n_meshes is not None:
            obj_list = obj_list[:n_meshes]
        obj_list = [os.path.join(mesh_dir, f) for f in obj_list]
    elif mesh_files is not None:
        obj_list = list(mesh_files)
    else:
        raise ValueError("Must specify either mesh_dir or mesh_files")
    names, all_v, all_f = [], [], []
    for p in obj_list:
        names.append(os.path.basename(p)[:-4])
        v, f = load_obj(p)
        v = v - v.mean(0)
        v = v / v.abs().max()
        all_v.append(v.to(device))
        all_f.append(f.to(device))
    return names, Meshes(verts=all_v, faces=all_f)


class Topology:
    """Regulariser tables of one (F,3) face array over V vertices (pytorch3d 0.7.8 semantics)."""

    def __init__(self, faces: np.ndarray, V: int):
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        self.V = int(V)
        F = f.shape[0]
        # face edges in pytorch3d's order (edges opposite corner 0, 1, 2), each sorted
        fe = np.concatenate([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], axis=0)  # (3F,2): row k*F + i is edge k of face i
        opp = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
        fe.sort(axis=1)
        key = fe[:, 0] * self.V + fe[:, 1]
        ukey, inv = np.unique(key, return_inverse=True)
        self.edges = np.stack([ukey // self.V, ukey % self.V], axis=1).astype(np.int64)
        self.E = len(self.edges)
        # normal pairs: faces sharing an edge, in face order, every pair i < j
        order = np.lexsort((np.tile(np.arange(F), 3), inv))  # by edge, then face
        o_sorted = opp[order]
        counts = np.bincount(inv, minlength=self.E)
        start = np.concatenate([[0], np.cumsum(counts)[:-1]])
        pairs = []
        two = np.nonzero(counts == 2)[0]
        if len(two):
            s = start[two]
            pairs.append(np.stack([self.edges[two, 0], self.edges[two, 1], o_sorted[s], o_sorted[s + 1]], axis=1))
        for e in np.nonzero(counts > 2)[0]:
            o = o_sorted[start[e]:start[e] + counts[e]]
            k = len(o)
            ii, jj = np.triu_indices(k, 1)
            pairs.append(np.stack([np.full(len(ii), self.edges[e, 0]), np.full(len(ii), self.edges[e, 1]), o[ii], o[jj]], axis=1))
        self.pairs = np.concatenate(pairs, axis=0).astype(np.int64) if pairs else np.zeros((0, 4), np.int64)
        self.Q = len(self.pairs)
        # Laplacian neighbour CSR
        rows = np.concatenate([self.edges[:, 0], self.edges[:, 1]])
        cols = np.concatenate([self.edges[:, 1], self.edges[:, 0]])
        o = np.lexsort((cols, rows))
        self.nbr = cols[o]
        deg = np.bincount(rows, minlength=self.V)
        self.nbr_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        self.deg = deg
        self.inv_deg = np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)
        # vertex -> pair incidence CSR (pair * 4 + role)
        code = np.arange(4 * self.Q, dtype=np.int64)
        owner = self.pairs.reshape(-1)
        o = np.argsort(owner, kind="stable")
        self.vpair = code[o]
        self.vpair_ptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=self.V))]).astype(np.int64)
        self._dev = {}

    def device(self, device) -> "engine.DeviceTopology":
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = engine.DeviceTopology(self, device)
        return self._dev[key]


_TOPOLOGY_CACHE = {}  # (V, faces bytes digest) -> Topology: built once per topology for every Meshes that shares it


def topology_for(faces: torch.Tensor, V: int) -> Topology:
    f = faces.detach().cpu().numpy().astype(np.int64)
    key = (int(V), f.shape, hashlib.sha1(f.tobytes()).hexdigest())
    if key not in _TOPOLOGY_CACHE:
        _TOPOLOGY_CACHE[key] = Topology(f, V)
    return _TOPOLOGY_CACHE[key]


class Meshes:
    """A batch of triangle meshes: ``verts`` / ``faces`` as lists of (V_n,3) / (F_n,3) tensors or padded (N,V,3) / (N,F,3) tensors.
    The subset of pytorch3d.structures.Meshes that fitter_3d/trainer.py uses."""

    def __init__(self, verts, faces, _shared: Optional[dict] = None):
        if isinstance(verts, torch.Tensor):
            if verts.dim() != 3 or not isinstance(faces, torch.Tensor) or faces.dim() != 3 or faces.shape[0] != verts.shape[0]:
                raise ValueError("padded verts (N,V,3) need padded faces (N,F,3)")
            self._verts_list = None
            self._padded = verts
            self._faces_padded = faces
        else:
            verts, faces = list(verts), list(faces)
            if len(verts) != len(faces) or not verts:
                raise ValueError("verts and faces must be non-empty lists of equal length")
            self._verts_list = verts
            self._faces_list = faces
            self._padded = None
        self._shared = _shared if _shared is not None else {}  # tables of the face arrays, kept by offset_verts()
        self._sampling = None  # the area table depends on the vertices: kept by this object only

    # ---- sizes / views -------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self._padded.shape[0]) if self._padded is not None else len(self._verts_list)

    @property
    def device(self):
        return self._padded.device if self._padded is not None else self._verts_list[0].device

    def verts_list(self) -> List[torch.Tensor]:
        return list(self._padded.unbind(0)) if self._verts_list is None else self._verts_list

    def faces_list(self) -> List[torch.Tensor]:
        return list(self._faces_padded.unbind(0)) if self._verts_list is None else self._faces_list

    def num_verts_per_mesh(self) -> List[int]:
        return [int(v.shape[0]) for v in self.verts_list()]

    def num_faces_per_mesh(self) -> List[int]:
        return [int(f.shape[0]) for f in self.faces_list()]

    def verts_padded(self) -> torch.Tensor:
        if self._padded is None:
            vl = self._verts_list
            Vmax = max(int(v.shape[0]) for v in vl)
            self._padded = torch.stack([torch.nn.functional.pad(v, (0, 0, 0, Vmax - v.shape[0])) for v in vl])
        return self._padded

    def verts_packed(self) -> torch.Tensor:
        return self._padded.reshape(-1, 3) if self._verts_list is None else torch.cat(self._verts_list, 0)

    def faces_packed(self) -> torch.Tensor:
        """(sum F_n, 3) indices into verts_packed()."""
        if "faces_packed" not in self._shared:
            off, out = 0, []
            for v, f in zip(self.verts_list(), self.faces_list()):
                out.append(f.to(torch.int64) + off)
                off += int(v.shape[0])
            self._shared["faces_packed"] = torch.cat(out, 0)
        return self._shared["faces_packed"]

    def offset_verts(self, vert_offsets_packed: torch.Tensor) -> "Meshes":
        """A new Meshes with verts_packed() + offsets (differentiable), the same faces and the cached tables."""
        if self._verts_list is None:
            return Meshes(self._padded + vert_offsets_packed.view(self._padded.shape), self._faces_padded, _shared=self._shared)
        new, off = [], 0
        for v in self._verts_list:
            n = int(v.shape[0])
            new.append(v + vert_offsets_packed[off:off + n])
            off += n
        return Meshes(new, self._faces_list, _shared=self._shared)

    def to(self, device) -> "Meshes":
        if self._verts_list is None:
            return Meshes(self._padded.to(device), self._faces_padded.to(device))
        return Meshes([v.to(device) for v in self._verts_list], [f.to(device) for f in self._faces_list])

    # ---- cached tables -------------------------------------------------------------------------------------------------------
    def topology(self) -> Topology:
        """The regulariser tables, when every mesh has the same face array and vertex count (fitter_3d's source meshes)."""
        if "topology" not in self._shared:
            fl, nv = self.faces_list(), self.num_verts_per_mesh()
            f0 = fl[0]
            if any(n != nv[0] for n in nv) or any(f.shape != f0.shape or not torch.equal(f, f0) for f in fl[1:]):
                raise NotImplementedError("the mesh regularisers need one face array shared by every mesh of the batch")
            self._shared["topology"] = topology_for(f0, nv[0])
        return self._shared["topology"]

    def face_tables(self) -> "engine.MeshTables":
        """The packed int32 faces with the face and vertex offsets of every mesh, as the point-mesh kernels take them: built from the
        shapes without a host synchronisation, cached with the face arrays (kept by offset_verts())."""
        if "face_tables" not in self._shared:
            nv, nf = self.num_verts_per_mesh(), self.num_faces_per_mesh()
            dev = self.device
            off = lambda counts: torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)  # noqa: E731
            self._shared["face_tables"] = engine.MeshTables(self.faces_packed().to(device=dev, dtype=torch.int32).contiguous(), off(nf),
                                                            off(nv), len(self), int(sum(nf)), int(max(nf)), int(sum(nv)), int(max(nv)))
        return self._shared["face_tables"]

    def sampling_tables(self):
        """(faces_packed int32, face_off int32, cum_area float64) on the device: per-mesh inclusive cumulative face areas divided
        by the mesh's total, computed on the host in float64 from the current vertices and cached (targets are fixed for a run)."""
        if self._sampling is None:
            dev = self.device
            fp, off, cum = [], [0], []
            voff = 0
            for v, f in zip(self.verts_list(), self.faces_list()):
                vv = v.detach().cpu().numpy().astype(np.float64)
                ff = f.detach().cpu().numpy().astype(np.int64)
                a = 0.5 * np.linalg.norm(np.cross(vv[ff[:, 1]] - vv[ff[:, 0]], vv[ff[:, 2]] - vv[ff[:, 0]]), axis=1)
                c = np.cumsum(a)
                cum.append(c / c[-1] if len(c) and c[-1] > 0 else np.zeros_like(c))
                fp.append(ff + voff)
                voff += len(vv)
                off.append(off[-1] + len(ff))
            self._sampling = (
                torch.from_numpy(np.concatenate(fp).astype(np.int32)).to(dev),
                torch.from_numpy(np.asarray(off, np.int32)).to(dev),
                torch.from_numpy(np.concatenate(cum)).to(dev))
        return self._sampling


ClosestPoints = namedtuple("ClosestPoints", "dist2 face bary points")


class MeshBVH:
    """A bounding-volume hierarchy over the faces of ``meshes`` (csrc/mesh_bvh.hip), built once on the GPU for
    meshes that do not change during a run: ``closest_points`` answers exactly as ``mesh3d.closest_points`` does - the same face, the
    same bits - but visits only the faces near each point.  ``refit(meshes)`` takes new vertices with the same faces and keeps the
    order; the answers stay exact however far the vertices moved, only the number of faces visited grows.  No host synchronisation at
    construction or after it.  ``sort_queries``: whether the queries are handed to the kernel in Morton order (the same answers)."""

    SORT_QUERIES = False  # the default of ``sort_queries``: the faster setting of tools/mesh_bvh_probe.py

    def __init__(self, meshes: Meshes, sort_queries: Optional[bool] = None):
        engine.require_gpu(meshes.device)
        self.sort_queries = self.SORT_QUERIES if sort_queries is None else bool(sort_queries)
        self._tables = meshes.face_tables()
        self._verts = meshes.verts_packed().detach().to(torch.float32).contiguous()
        self._order, self._boxes = engine.bvh_build(self._verts, self._tables)
        self._face_off_host = np.concatenate([[0], np.cumsum(meshes.num_faces_per_mesh())]).tolist()

    def _check(self, meshes: Meshes) -> "engine.MeshTables":
        """The tables of ``meshes``, which must have this hierarchy's face arrays (the same object, or the same sizes: the contents
        are the caller's statement, as ``refit`` documents)."""
        mt, own = meshes.face_tables(), self._tables
        if mt is not own and (mt.n_meshes, mt.n_faces, mt.max_faces, mt.n_verts, mt.max_verts) != \
                (own.n_meshes, own.n_faces, own.max_faces, own.n_verts, own.max_verts):
            raise ValueError("MeshBVH: these are not the meshes the hierarchy was built for (other face or vertex counts)")
        return own

    def refit(self, meshes: Meshes) -> "MeshBVH":
        """New vertices, the same faces (``offset_verts`` of the built meshes, or meshes of equal face arrays - that they are equal is
        the caller's statement): every box is recomputed in the stored order, without a sort."""
        self._check(meshes)
        self._verts = meshes.verts_packed().detach().to(torch.float32).contiguous()
        engine.bvh_refit(self._verts, self._tables, self._order, self._boxes)
        return self

    def query(self, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, want_evaluated: bool = False, verts=None):
        """(dist2, face int32, bary, evaluated or None) of ``engine.bvh_point_face_distance`` on the hierarchy's vertices (``verts``:
        the same values with another history, for autograd)."""
        return engine.bvh_point_face_distance(self._verts if verts is None else verts, self._tables, self._order, self._boxes, points, lengths,
                                              self.sort_queries, want_evaluated)

    def closest_points(self, points: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> "ClosestPoints":
        """``mesh3d.closest_points`` of the built (or refitted) meshes, bit for bit."""
        pts = points.detach().to(device=self._verts.device, dtype=torch.float32).contiguous()
        dist2, face, bary, _ = self.query(pts, lengths)
        return _closest(self._verts, self._tables, dist2, face, bary)

    def evaluated(self, points: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N,P) int32: how many leaf faces the search evaluated for every point (the brute force evaluates every face)."""
        return self.query(points.detach().to(device=self._verts.device, dtype=torch.float32).contiguous(), lengths, True)[3]

    def arrays(self) -> dict:
        """For inspection: ``order`` (F_total) int32, sorted position -> face within its mesh, mesh n's positions at
        ``face_off[n]`` ..; ``boxes`` (nodes,6) float32, lo xyz and hi xyz; and per mesh, from the shapes alone (host lists):
        ``node0`` (row of ``boxes`` that heap index 0 would take: node i is row node0 + i, the root is 1), ``leaves`` (L) and
        ``padded_leaves`` (Lp, a power of two: leaf k is node Lp + k and holds the sorted positions k * leaf_size ..) and
        ``leaf_size``."""
        leaf = int(engine._lib.BVH_LEAF)
        nf = [int(b) - int(a) for a, b in zip(self._face_off_host[:-1], self._face_off_host[1:])]
        L = [-(-f // leaf) for f in nf]
        Lp = [1 << max(l - 1, 0).bit_length() for l in L]
        node0 = [4 * (int(f0) // leaf + n) for n, f0 in enumerate(self._face_off_host[:-1])]
        return dict(order=self._order, boxes=self._boxes, node0=node0, leaves=L, padded_leaves=Lp, leaf_size=leaf)


def _closest(verts, mt, dist2, face, bary) -> "ClosestPoints":
    face = face.long()
    first = mt.face_off[:-1].long()[:, None]
    tri = verts[mt.faces.long()[(face.clamp(min=0) + first)]]  # (N,P,3,3)
    return ClosestPoints(dist2, face, bary, (bary[..., None] * tri).sum(-2))


def closest_points(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, bvh: Optional[MeshBVH] = None) -> ClosestPoints:
    """For every point of ``points`` (N,P,3) the closest point of the surface of its mesh: squared distance (N,P), face within the mesh
    (N,P) int64, barycentrics (N,P,3) and the closest points themselves (N,P,3).  ``dist2.sqrt()`` is the surface error per point - the
    registration metric.  Exact (the true Euclidean distance to the closed triangles, a brute-force search over every face, the value
    in float64); not differentiable (``fit3d.point_face_distance`` is); no host synchronisation.  ``lengths`` (N): points at or beyond
    a cloud's length, non-finite points and meshes without a usable face give ``inf``, face -1 and zeros.  ``bvh``: a ``MeshBVH`` of
    these meshes (built or refitted on these vertices): the same result, bit for bit, through the hierarchy."""
    engine.require_gpu(meshes.device)
    verts = meshes.verts_packed().detach().to(torch.float32).contiguous()
    pts = points.detach().to(device=verts.device, dtype=torch.float32).contiguous()
    mt = meshes.face_tables()
    if bvh is not None:
        bvh._check(meshes)
        dist2, face, bary, _ = bvh.query(pts, lengths, verts=verts)
    else:
        dist2, face, bary = engine.point_mesh_distance(verts, mt, pts, lengths)
    return _closest(verts, mt, dist2, face, bary)


SignedDistance = namedtuple("SignedDistance", "sdist dist2 face bary points winding")


def winding_number(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The generalised winding number (N,P) float32 of every point of ``points`` (N,P,3) with respect to its mesh (Jacobson et al.
    2013): the sum over all faces of the signed solid angle / (4 pi).  1 inside a closed mesh with outward faces, 0 outside, -1 inside
    one with inward faces, k inside k nested shells; on open or self-intersecting meshes a smooth function near those integers away
    from the defects.  A face seen edge-on (its determinant is +-0: a point in its plane or on a vertex, a degenerate face) adds 0.
    Points at or beyond ``lengths`` (N) and non-finite points give NaN; a mesh without faces gives 0.  A brute-force sum, integer
    accumulated: the same bits whatever the order of the faces.  Not differentiable; no host synchronisation."""
    engine.require_gpu(meshes.device)
    verts = meshes.verts_packed().detach().to(torch.float32).contiguous()
    pts = points.detach().to(device=verts.device, dtype=torch.float32).contiguous()
    return engine.point_mesh_winding(verts, meshes.face_tables(), pts, lengths)


def _inside(winding: torch.Tensor, oriented: bool) -> torch.Tensor:
    return (winding if oriented else winding.abs()) > 0.5  # (NaN compares false)


def contains(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, oriented: bool = True) -> torch.Tensor:
    """(N,P) bool: whether each point lies inside its mesh: ``winding_number > 0.5``, or ``|winding_number| > 0.5`` with
    ``oriented=False`` (scans whose faces point inwards).  False where the winding number is NaN."""
    return _inside(winding_number(meshes, points, lengths), oriented)


def signed_distance(meshes: Meshes, points: torch.Tensor, lengths: Optional[torch.Tensor] = None, oriented: bool = True, *,
                    bvh: Optional[MeshBVH] = None) -> SignedDistance:
    """``closest_points`` with a sign: ``sdist`` (N,P) = -sqrt(dist2) where ``contains`` says inside, +sqrt(dist2) elsewhere, +inf where
    ``closest_points`` gives inf; then its dist2, face, bary and points, and the winding number that decided.  Not differentiable
    (``fit3d.point_mesh_signed_distance`` is).  ``bvh``: as in ``closest_points``, for the distance; the winding number stays the
    brute-force sum over all faces."""
    cp = closest_points(meshes, points, lengths, bvh=bvh)
    w = winding_number(meshes, points, lengths)
    d = cp.dist2.sqrt()
    return SignedDistance(torch.where(_inside(w, oriented), -d, d), cp.dist2, cp.face, cp.bary, cp.points, w)
