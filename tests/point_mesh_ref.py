"""A restatement of the point <-> triangle-mesh distances of smilify_amd/csrc/point_mesh.hip in torch tensor operations (float64
unless handed something else), for tests: it defines what the kernels compute, it is slow, and it runs anywhere.

* ``closest_on_triangle(p, tri)``: the closest point of the closed triangle by its seven Voronoi regions, tried in the order A, B, AB,
  C, AC, BC, interior (Ericson, Real-Time Collision Detection, 5.1.5), with the kernel's two additions for degenerate faces: an edge
  region also asks that its denominator (the edge's squared length in exact arithmetic) is > 0, and the interior's ratios are clamped
  to the triangle.  An edge of zero length then acts as its end point, a face of zero area as the nearest of its three segments and
  three equal vertices as a point.  Differentiable: usable under autograd at GIVEN pairs.
* ``all_pairs`` / ``point_face`` / ``face_point``: brute force over every (point, face) pair of one mesh, the first minimum.
* ``dist2_at`` / ``gradients_at``: the squared distance of given pairs, and its analytic gradient 2 g e, -2 g b_k e.
* ``loss``: pytorch3d's point_mesh_face_distance normalisation.
* ``dist2_independent``: a second formulation that shares no region logic: the plane distance when the projection falls inside
  the triangle, else the smallest of the three segment distances.
"""
import numpy as np
import torch

U = 2.0 ** -24  # half an ulp of 1 in float32
USABLE = 3.0e38  # a coordinate above this in magnitude counts as non-finite, for vertices and points alike


def closest_on_triangle(p: torch.Tensor, tri: torch.Tensor):
    """p (..., 3), tri (..., 3, 3) -> (bary (..., 3), dist2 (...)): the closest point is sum_k bary_k tri_k."""
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    e1, e2, ap = b - a, c - a, p - a
    bp, cp = ap - e1, ap - e2
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(e1, ap), dot(e2, ap), dot(e1, bp), dot(e2, bp), dot(e1, cp), dot(e2, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    ab_den, ac_den, bc_n, bc_m = d1 - d3, d2 - d6, d4 - d3, d5 - d6
    bc_den = bc_n + bc_m
    in_a = (d1 <= 0) & (d2 <= 0)
    in_b = (d3 >= 0) & (d4 <= d3)
    in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (ab_den > 0)
    in_c = (d6 >= 0) & (d5 <= d6)
    in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (ac_den > 0)
    in_bc = (va <= 0) & (bc_n >= 0) & (bc_m >= 0) & (bc_den > 0)
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    safe = lambda den: torch.where(den > 0, den, one)  # noqa: E731  (a branch that is not selected must not put NaN into a gradient)
    den = va + vb + vc
    ok = den > 0
    v = torch.where(ok, vb / safe(den), zero).clamp(0, 1)  # interior (0 / 0 clamps to 0, as the kernel's NaN does)
    w = torch.minimum(torch.where(ok, vc / safe(den), zero).clamp(min=0), 1 - v)
    b0 = (1 - v) - w
    t = (bc_n / safe(bc_den)).clamp(0, 1)
    b0, v, w = torch.where(in_bc, zero, b0), torch.where(in_bc, 1 - t, v), torch.where(in_bc, t, w)
    t = (d2 / safe(ac_den)).clamp(0, 1)
    b0, v, w = torch.where(in_ac, 1 - t, b0), torch.where(in_ac, zero, v), torch.where(in_ac, t, w)
    b0, v, w = torch.where(in_c, zero, b0), torch.where(in_c, zero, v), torch.where(in_c, one, w)
    t = (d1 / safe(ab_den)).clamp(0, 1)
    b0, v, w = torch.where(in_ab, 1 - t, b0), torch.where(in_ab, t, v), torch.where(in_ab, zero, w)
    b0, v, w = torch.where(in_b, zero, b0), torch.where(in_b, one, v), torch.where(in_b, zero, w)
    b0, v, w = torch.where(in_a, one, b0), torch.where(in_a, zero, v), torch.where(in_a, zero, w)
    r = ap - v[..., None] * e1 - w[..., None] * e2
    return torch.stack([b0, v, w], -1), dot(r, r)


def region(p, tri) -> str:
    """The name of the region that decides for ONE point and triangle (hand cases)."""
    bary, _ = closest_on_triangle(torch.as_tensor(p, dtype=torch.float64), torch.as_tensor(tri, dtype=torch.float64))
    on = [bool(x > 0) for x in bary]
    return {(True, False, False): "A", (False, True, False): "B", (False, False, True): "C", (True, True, False): "AB",
            (True, False, True): "AC", (False, True, True): "BC", (True, True, True): "interior"}[tuple(on)]


def _f64(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(torch.float64)


def _idx(x, like: torch.Tensor) -> torch.Tensor:
    """An index array on the device of ``like`` (the restatement runs wherever its inputs are)."""
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).long().to(like.device)


def all_pairs(verts, faces, points, chunk: int = 256) -> torch.Tensor:
    """dist2 (P, F) of every point to every face of one mesh, float64.  A face with a non-finite vertex and a non-finite point: inf
    (a coordinate above 3e38 in magnitude counts as non-finite)."""
    v, pts = _f64(verts), _f64(points)
    tri = v[_idx(faces, v)]  # (F,3,3)
    out = []
    for s in range(0, len(pts), chunk):
        _, d = closest_on_triangle(pts[s:s + chunk, None, :], tri[None])
        out.append(d)
    d = torch.cat(out) if out else torch.zeros(0, len(tri), dtype=torch.float64, device=v.device)
    usable = (pts.abs() <= USABLE).all(-1)[:, None] & (tri.abs() <= USABLE).all(-1).all(-1)[None]  # (NaN compares false)
    return torch.where(torch.isfinite(d) & usable, d, torch.full_like(d, float("inf")))


def _first_min(d: torch.Tensor, dim: int):
    """(values, indices) of the first minimum along dim; -1 where it is inf or the axis is empty."""
    if d.shape[dim] == 0:
        shape = d.shape[:dim] + d.shape[dim + 1:]
        return (torch.full(shape, float("inf"), dtype=torch.float64, device=d.device),
                torch.full(shape, -1, dtype=torch.int64, device=d.device))
    val = d.min(dim).values
    first = (d == val.unsqueeze(dim)).to(torch.uint8).argmax(dim)  # argmax returns the first of equal values
    return val, torch.where(torch.isfinite(val), first, torch.full_like(first, -1))


def point_face(verts, faces, points):
    """(dist2 (P), face (P)) of one mesh: the nearest face of every point, the smaller index on a float64 tie."""
    return _first_min(all_pairs(verts, faces, points), 1)


def face_point(verts, faces, points):
    """(dist2 (F), point (F)) of one mesh: the nearest point of every face."""
    return _first_min(all_pairs(verts, faces, points), 0)


def dist2_at(verts, faces, points, face_idx, point_idx=None):
    """(bary, dist2) of given pairs of one mesh: point point_idx[r] (default r) against face face_idx[r].  Tensors keep their dtype and
    their graph: under autograd this is the loss at fixed indices."""
    v = verts if isinstance(verts, torch.Tensor) else _f64(verts)
    p = points if isinstance(points, torch.Tensor) else _f64(points)
    tri = v[_idx(faces, v)[_idx(face_idx, v)]]
    if point_idx is not None:
        p = p[_idx(point_idx, v)]
    return closest_on_triangle(p, tri)


def gradients_at(verts, faces, points, face_idx, g, point_idx=None):
    """The analytic gradient of sum_r g_r dist2_r at given pairs in float64: (d_points (P,3), d_verts (V,3)); with e = p - c,
    2 g e to the point and -2 g b_k e to vertex k of the face."""
    v, p, g = _f64(verts), _f64(points), _f64(g)
    f = _idx(faces, v)[_idx(face_idx, v)]
    pi = torch.arange(len(face_idx), device=v.device) if point_idx is None else _idx(point_idx, v)
    bary, _ = closest_on_triangle(p[pi], v[f])
    e = p[pi] - (bary[..., None] * v[f]).sum(-2)
    ge = 2.0 * g[:, None] * e
    d_points = torch.zeros_like(p).index_add_(0, pi, ge)
    d_verts = torch.zeros_like(v)
    for k in range(3):
        d_verts.index_add_(0, f[:, k], -bary[:, k:k + 1] * ge)
    return d_points, d_verts


def loss(meshes, clouds) -> float:
    """point_mesh_face_distance of a batch: meshes [(verts, faces)], clouds [points (P_n,3)]: the mean over each cloud's points of the
    point -> face term plus the mean over each mesh's faces of the face -> point term, averaged over the batch; inf entries add 0."""
    total = 0.0
    for (v, f), pts in zip(meshes, clouds):
        d = all_pairs(v, f, pts)
        pf, fp = _first_min(d, 1)[0], _first_min(d, 0)[0]
        pf, fp = torch.where(torch.isfinite(pf), pf, torch.zeros_like(pf)), torch.where(torch.isfinite(fp), fp, torch.zeros_like(fp))
        total += float(pf.sum()) / max(len(pts), 1) + float(fp.sum()) / max(len(f), 1)
    return total / len(meshes)


# ---- the second, independent formulation ------------------------------------------------------------------------------------------
def _segment_dist2(p, a, b):
    ab = b - a
    l2 = (ab * ab).sum(-1)
    t = torch.where(l2 > 0, ((p - a) * ab).sum(-1) / torch.where(l2 > 0, l2, torch.ones_like(l2)), torch.zeros_like(l2)).clamp(0, 1)
    r = p - (a + t[..., None] * ab)
    return (r * r).sum(-1)


def dist2_independent(p: torch.Tensor, tri: torch.Tensor) -> torch.Tensor:
    """The squared distance without the region walk: the foot of the perpendicular on the triangle's plane when its barycentrics
    (solved from the 2 x 2 Gram system) are all >= 0, else the smallest of the three segment distances.  Zero-area faces: segments."""
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    e1, e2, ap = b - a, c - a, p - a
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    r1, r2 = (e1 * ap).sum(-1), (e2 * ap).sum(-1)
    det = g11 * g22 - g12 * g12
    ok = det > 1e-30 * (g11 * g22 + 1e-300)
    sdet = torch.where(ok, det, torch.ones_like(det))
    v, w = (g22 * r1 - g12 * r2) / sdet, (g11 * r2 - g12 * r1) / sdet
    inside = ok & (v >= 0) & (w >= 0) & (v + w <= 1)
    n = torch.linalg.cross(e1, e2)
    n2 = (n * n).sum(-1)
    plane = (n * ap).sum(-1) ** 2 / torch.where(n2 > 0, n2, torch.ones_like(n2))
    seg = torch.minimum(torch.minimum(_segment_dist2(p, a, b), _segment_dist2(p, a, c)), _segment_dist2(p, b, c))
    return torch.where(inside, torch.minimum(plane, seg), seg)


# ---- the selection bound --------------------------------------------------------------------------------
def shape_factor(verts, faces) -> torch.Tensor:
    """kappa (F) = (longest edge)^2 / area of every face, float64 (equilateral: 4 / sqrt 3 = 2.31; inf for a face of zero area)."""
    v = _f64(verts)
    tri = v[_idx(faces, v)]
    e = torch.stack([((tri[:, i] - tri[:, (i + 1) % 3]) ** 2).sum(-1) for i in range(3)], -1).max(-1).values
    area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1)
    return torch.where(area > 0, e / torch.where(area > 0, area, torch.ones_like(area)), torch.full_like(area, float("inf")))


def longest_edge(verts, faces) -> torch.Tensor:
    v = _f64(verts)
    tri = v[_idx(faces, v)]
    return torch.stack([(tri[:, i] - tri[:, (i + 1) % 3]).norm(dim=-1) for i in range(3)], -1).max(-1).values


def selection_c(kappa: torch.Tensor) -> torch.Tensor:
    """c of the bound d(selected) - min_f d(f) <= c u L for a pair of faces whose larger shape factor is kappa: 13 + 40 kappa^2."""
    return 13.0 + 40.0 * kappa ** 2


def selection_bound(kappa: torch.Tensor, edge: torch.Tensor, L: torch.Tensor) -> torch.Tensor:
    """The bound on d(selected) - min_f d(f) for a pair of faces with the larger shape factor kappa and the longer longest edge
    `edge`: 13 u L of evaluation plus the parameter error, 40 kappa^2 u L but never more than the face's own longest edge (the
    computed point is ON the face, wherever its parameters went): finite for a face of zero area too."""
    return 13.0 * U * L + torch.minimum(40.0 * kappa ** 2 * U * L, edge)
