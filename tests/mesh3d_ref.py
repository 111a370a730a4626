"""Float64 CPU restatement of the 3-D registration losses (pytorch3d 0.7.8 semantics, which is not installed here to compare with):

* chamfer_distance(x, y), norm 2, no lengths: red_n [ red_i min_j |x_i - y_j|^2 + red_j min_i |y_j - x_i|^2 ] by brute force;
* mesh_edge_loss (target 0): per-mesh mean over the unique edges of |v0 - v1|^2, then the mean over meshes;
* mesh_normal_consistency: for every edge and every pair i < j of the faces that share it, with a, b the faces' opposite vertices,
  n0 = e x (a - v0), n1 = -e x (b - v0), e = v1 - v0, the term 1 - torch.cosine_similarity(n0, n1); per-mesh mean over pairs, then
  the mean over meshes;
* mesh_laplacian_smoothing("uniform"): L[i,j] = 1/deg(i) for each edge neighbour, L[i,i] = -1; per-mesh mean of |(L V)_i|, then
  the mean over meshes.

Edges and pairs are found by brute force from the faces (not from smilify_amd.mesh3d.Topology).  Gradients: float64 autograd.
"""
from collections import defaultdict

import numpy as np
import torch


def edges_brute(faces):
    s = set()
    for a, b, c in np.asarray(faces).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            s.add((min(u, v), max(u, v)))
    return np.array(sorted(s), np.int64).reshape(-1, 2)


def normal_pairs_brute(faces):
    opp = defaultdict(list)
    for a, b, c in np.asarray(faces).tolist():
        for (u, v), o in (((b, c), a), ((c, a), b), ((a, b), c)):
            opp[(min(u, v), max(u, v))].append(o)
    out = []
    for (u, v), os_ in sorted(opp.items()):
        for i in range(len(os_)):
            for j in range(i + 1, len(os_)):
                out.append((u, v, os_[i], os_[j]))
    return np.array(out, np.int64).reshape(-1, 4)


def chamfer(x, y, single_directional=False, point_sum=False, batch_sum=False):
    """x (N,P1,3), y (N,P2,3) float64 -> loss, idx_x (N,P1), idx_y (N,P2)."""
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)  # (N,P1,P2)
    dx, ix = d.min(2)
    dy, iy = d.min(1)
    rx = dx.sum(1) if point_sum else dx.mean(1)
    ry = dy.sum(1) if point_sum else dy.mean(1)
    per = rx if single_directional else rx + ry
    return (per.sum() if batch_sum else per.mean()), ix, iy


def chamfer_at(x, y, ix, iy, single_directional=False):
    """The mean/mean chamfer loss with the argmins fixed at ix, iy (its gradient is the chamfer gradient at those indices)."""
    yx = torch.gather(y, 1, ix[..., None].expand(-1, -1, 3))
    l = ((x - yx) ** 2).sum(-1).mean(1)
    if not single_directional:
        xy = torch.gather(x, 1, iy[..., None].expand(-1, -1, 3))
        l = l + ((y - xy) ** 2).sum(-1).mean(1)
    return l.mean()


def edge_loss(verts, faces):
    e = torch.from_numpy(edges_brute(faces))
    d = verts[:, e[:, 0]] - verts[:, e[:, 1]]
    return (d.norm(dim=-1) ** 2).mean(1).mean()


def normal_loss(verts, faces):
    p = torch.from_numpy(normal_pairs_brute(faces))
    if len(p) == 0:
        return verts.sum() * 0
    v0, v1, a, b = (verts[:, p[:, k]] for k in range(4))
    e = v1 - v0
    n0 = torch.cross(e, a - v0, dim=-1)
    n1 = -torch.cross(e, b - v0, dim=-1)
    return (1 - torch.cosine_similarity(n0, n1, dim=-1)).mean(1).mean()


def laplacian_loss(verts, faces):
    V = verts.shape[1]
    e = edges_brute(faces)
    L = torch.zeros(V, V, dtype=verts.dtype)
    deg = np.bincount(e.reshape(-1), minlength=V)
    for u, v in e.tolist():
        L[u, v] = 1.0 / deg[u]
        L[v, u] = 1.0 / deg[v]
    L -= torch.eye(V, dtype=verts.dtype)
    r = torch.einsum("ij,bjc->bic", L, verts)
    return r.norm(dim=-1).mean(1).mean()


def laplacian_loss_sparse(verts, faces):
    """laplacian_loss for large V (no dense V x V matrix)."""
    V = verts.shape[1]
    e = torch.from_numpy(edges_brute(faces))
    rows = torch.cat([e[:, 0], e[:, 1]])
    cols = torch.cat([e[:, 1], e[:, 0]])
    deg = torch.bincount(rows, minlength=V).to(verts.dtype)
    s = torch.zeros_like(verts).index_add_(1, rows, verts[:, cols])
    inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))
    r = s * inv[None, :, None] - verts
    return r.norm(dim=-1).mean(1).mean()


def with_grad(fn, verts, *args):
    v = verts.detach().to(torch.float64).clone().requires_grad_(True)
    loss = fn(v, *args)
    (g,) = torch.autograd.grad(loss, v)
    return float(loss), g
