"""Float64 CPU restatement of the 3-D registration losses (pytorch3d 0.7.8 semantics, which is not installed here to compare with):

* chamfer_distance(x, y), norm 2, no lengths: red_n [ red_i min_j |x_i - y_j|^2 + red_j min_i |y_j - x_i|^2 ] by brute force;
* mesh_edge_loss (target 0): per-mesh mean over the unique edges of |v0 - v1|^2, then the mean over meshes;
* mesh_normal_consistency: for every edge and every pair i < j of the faces that share it, with a, b the faces' opposite vertices,
  n0 = e x (a - v0), n1 = -e x (b - v0), e = v1 - v0, the term 1 - torch.cosine_similarity(n0, n1); per-mesh mean over pairs, then
  the mean over meshes;
* mesh_laplacian_smoothing("uniform"): L[i,j] = 1/deg(i) for each edge neighbour, L[i,i] = -1; per-mesh mean of |(L V)_i|, then
  the mean over meshes.

Edges and pairs are found by brute force from the faces (not from smilify_amd.mesh3d.Topology).  Gradients: float64 autograd.

For the kernel-level tests (tests/test_gpu_mesh3d_kernels.py): ``philox4x32_10`` / ``sample_points`` restate the surface sampler
step by step (exact integers and float64, the barycentric weights in numpy float32); ``chamfer_brute`` is the chunked float64
nearest-neighbour search with numpy's first-occurrence argmin, ``chamfer_grad_parts`` the owned and scattered halves of the chamfer
gradient; ``dyadic_clouds`` draws clouds on which float32 is exact; ``hand_meshes`` are the regulariser edge cases.
"""
import functools
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


def chamfer_at(x, y, ix, iy, single_directional=False, point_sum=False, batch_sum=False):
    """The chamfer loss with the argmins fixed at ix, iy (its gradient is the chamfer gradient at those indices)."""
    red = (lambda t: t.sum(1)) if point_sum else (lambda t: t.mean(1))
    yx = torch.gather(y, 1, ix[..., None].expand(-1, -1, 3))
    l = red(((x - yx) ** 2).sum(-1))
    if not single_directional:
        xy = torch.gather(x, 1, iy[..., None].expand(-1, -1, 3))
        l = l + red(((y - xy) ** 2).sum(-1))
    return l.sum() if batch_sum else l.mean()


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
    return float(loss.detach()), g


# ---- surface sampler, restated ---------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011).  counter: four, key: two 32-bit words, each a Python integer or an array; returns
    the four output words as numpy uint64 (values < 2^32)."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _M32 for v in key]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & _M32, (k[1] + np.uint64(0xBB67AE85)) & _M32]
    return tuple(c)


def sample_draws(n, S, seed):
    """The three uniforms of samples 0 .. S-1 of mesh n: counter (s, n, 0, 0), key (seed lo, seed hi); uf float64 from 53 bits of
    words 0 and 1 (face choice), u and v float32 from the top 24 bits of words 2 and 3 (barycentrics).  All exact."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((np.arange(S, dtype=np.uint64), np.full(S, n, np.uint64), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    uf = ((r[0] << np.uint64(21)) ^ (r[1] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
    u = (r[2] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    v = (r[3] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return uf, u, v


def sample_points(verts_packed_f32, faces_packed, face_off, cum, S, seed):
    """k_sample_points step by step.  verts_packed_f32 (V,3) float32, faces_packed (F,3) into it, face_off (N+1), cum (F) float64
    per-mesh normalised cumulative areas -> (points (N,S,3) float64 from the float32 weights, face within its mesh (N,S) int64,
    max |coordinate| of each sample's face (N,S) float64).  A mesh without faces or without area: zeros, face -1."""
    verts = np.asarray(verts_packed_f32)
    assert verts.dtype == np.float32
    faces = np.asarray(faces_packed, np.int64).reshape(-1, 3)
    face_off = np.asarray(face_off, np.int64)
    cum = np.asarray(cum, np.float64)
    N = len(face_off) - 1
    pts = np.zeros((N, S, 3), np.float64)
    face = np.full((N, S), -1, np.int64)
    fmax = np.zeros((N, S), np.float64)
    for n in range(N):
        f0, f1 = int(face_off[n]), int(face_off[n + 1])
        if f1 <= f0 or not cum[f1 - 1] > 0.0:
            continue
        uf, u, v = sample_draws(n, S, seed)
        # the first face of the mesh with cum > uf (the search never leaves [f0, f1 - 1])
        lo = np.minimum(np.searchsorted(cum[f0:f1], uf, side="right"), f1 - f0 - 1)
        su = np.sqrt(u)
        assert su.dtype == np.float32
        w0, w1, w2 = np.float32(1) - su, su * (np.float32(1) - v), su * v
        tri = verts[faces[f0 + lo]].astype(np.float64)  # (S,3,3)
        pts[n] = (w0.astype(np.float64)[:, None] * tri[:, 0] + w1.astype(np.float64)[:, None] * tri[:, 1]
                  + w2.astype(np.float64)[:, None] * tri[:, 2])
        face[n] = lo
        fmax[n] = np.abs(tri).max((1, 2))
    return pts, face, fmax


# ---- chamfer: brute force with a documented tie rule, the gradient's two halves ----------------------------------------------------
def _nn_brute(q, c, chunk=256):
    """q (Pq,3), c (Pc,3) float64 -> (min squared distance (Pq), numpy first-occurrence argmin (Pq), number of minima (Pq))."""
    dmin, idx, cnt = np.empty(len(q)), np.empty(len(q), np.int64), np.empty(len(q), np.int64)
    for i in range(0, len(q), chunk):
        d = ((q[i:i + chunk, None, :] - c[None, :, :]) ** 2).sum(-1)
        idx[i:i + chunk] = np.argmin(d, axis=1)
        dmin[i:i + chunk] = d.min(1)
        cnt[i:i + chunk] = (d == dmin[i:i + chunk, None]).sum(1)
    return dmin, idx, cnt


def chamfer_brute(x, y):
    """x (N,P1,3), y (N,P2,3) -> dict of float64 / int64 numpy arrays: dx, ix, nx (ties) of x's points in y, and dy, iy, ny."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    a = [_nn_brute(x[n], y[n]) for n in range(len(x))]
    b = [_nn_brute(y[n], x[n]) for n in range(len(x))]
    out = {k: np.stack([t[j] for t in a]) for j, k in enumerate(("dx", "ix", "nx"))}
    out.update({k: np.stack([t[j] for t in b]) for j, k in enumerate(("dy", "iy", "ny"))})
    return out


def chamfer_weights(N, P1, P2, point_sum, batch_sum):
    bw = 1.0 if batch_sum else 1.0 / N
    return (1.0 if point_sum else 1.0 / P1) * bw, (1.0 if point_sum else 1.0 / P2) * bw


def chamfer_loss_from(dx, dy, single_directional, point_sum, batch_sum):
    w0, w1 = chamfer_weights(dx.shape[0], dx.shape[1], dy.shape[1], point_sum, batch_sum)
    return w0 * dx.sum() + (0.0 if single_directional else w1 * dy.sum())


def chamfer_grad_parts(x, y, ix, iy, single_directional=False, point_sum=False, batch_sum=False):
    """The float64 chamfer gradient at the indices ix, iy in its two halves: (own_x, sc_x, own_y, sc_y), d_x = own_x + sc_x.
    own: 2 w (q - c*) of the point's own term; sc: the sum of 2 w' (c - q) over the other cloud's queries that chose the point."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    w0, w1 = chamfer_weights(N, P1, P2, point_sum, batch_sum)
    own_x, sc_x, own_y, sc_y = np.zeros_like(x), np.zeros_like(x), np.zeros_like(y), np.zeros_like(y)
    for n in range(N):  # (the differences are summed before the weight is applied: on dyadic inputs the sums are then exact)
        e = x[n] - y[n][ix[n]]
        own_x[n] = 2 * w0 * e
        np.add.at(sc_y[n], ix[n], -e)
        if not single_directional:
            e = y[n] - x[n][iy[n]]
            own_y[n] = 2 * w1 * e
            np.add.at(sc_x[n], iy[n], -e)
    return own_x, 2 * w1 * sc_x, own_y, 2 * w0 * sc_y


CH_BLOCK_QPT, CH_TILE = 1024, 256  # k_chamfer_nn: query points per workgroup, candidates per LDS tile


def chamfer_splits(N, P1, P2, single_directional=False):
    """The host's candidate split count, and the candidates per split of the direction whose candidates number Pc."""
    dirs = 1 if single_directional else 2
    qblocks = -(-max(P1, P2) // CH_BLOCK_QPT)
    return max(1, min(min(P1, P2) // (4 * CH_TILE), -(-2048 // (qblocks * N * dirs))))


def chamfer_chunk(Pc, splits):
    return -(-(-(-Pc // splits)) // CH_TILE) * CH_TILE


@functools.lru_cache(maxsize=None)
def dyadic_clouds(N, P1, P2, seed=0):
    """Two clouds of multiples of 1/8 in [-1, 1]^3 (17^3 cells) as float32 numpy arrays: every difference, square and sum of three
    squares is exact in float32, and duplicates (exact ties) are frequent."""
    rng = np.random.RandomState(1000 * seed + 7 * N + 3 * P1 + P2)
    x = (rng.randint(-8, 9, size=(N, P1, 3)) / 8.0).astype(np.float32)
    y = (rng.randint(-8, 9, size=(N, P2, 3)) / 8.0).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def dyadic_reference(N, P1, P2, seed=0):
    """chamfer_brute of dyadic_clouds (computed once, shared, read-only)."""
    out = chamfer_brute(*dyadic_clouds(N, P1, P2, seed))
    for v in out.values():
        v.setflags(write=False)
    return out


DYADIC_SHAPES = [  # (N, P1, P2, single_directional, expected splits)
    (1, 1, 1, False, 1), (1, 1, 257, False, 1), (3, 5, 2500, False, 1), (2, 255, 256, False, 1), (2, 257, 1023, False, 1),
    (1, 1024, 1025, False, 1), (3, 2048, 2100, False, 2), (1, 3100, 5000, False, 3), (1, 4100, 4100, False, 4),
    (1, 4100, 4100, True, 4)]
TIE_QUOTA_MIN_P = 1024  # shapes whose smaller cloud has at least this many points must have >= 10 % tied queries


def tie_fraction(r, single_directional=False):
    n = (r["nx"] >= 2).sum() + (0 if single_directional else (r["ny"] >= 2).sum())
    return n / (r["nx"].size + (0 if single_directional else r["ny"].size))


# ---- regulariser edge cases ---------------------------------------------------------------------------------------------------
def tri_grid(nx, ny, extra=0, seed=None, offset=0.0):
    """A triangulated nx x ny grid of unit cells, flat (integer coordinates, z = 0) or, with ``seed``, every coordinate moved by up
    to 0.2 (so that no Laplacian residual is 0), translated by ``offset``, plus ``extra`` unreferenced vertices
    -> (verts (V,3) float32, faces (F,3) int64)."""
    xs, ys = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(nx * ny)], 1)
    if seed is not None:
        v = v + np.random.RandomState(seed).uniform(-0.2, 0.2, v.shape)
    v = v + offset
    v = np.concatenate([v, np.arange(1, extra + 1)[:, None] * np.array([[0.5, -0.25, 2.0]])], 0)
    f = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            f += [[a, b, c], [a, c, d]]
    return v.astype(np.float32), np.array(f, np.int64)


FOLD_SIN, FOLD_COS = float(np.float32(np.sqrt(3.0) / 2)), 0.5  # the folded pair's second apex: 60 degrees out of the plane


def hand_meshes():
    """name -> (verts (V,3) float32, faces (F,3) int64): the edge cases of k_mesh_reg."""
    f32 = lambda a: np.array(a, np.float32)  # noqa: E731
    i64 = lambda a: np.array(a, np.int64)  # noqa: E731
    m = {}
    m["triangle"] = (f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), i64([[0, 1, 2]]))  # E = 3, Q = 0
    m["tetrahedron"] = (f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), i64([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
    # two triangles on the edge (0, 1): n0 = (0, 0, 1), n1 = (0, sin, cos), so the one term is 1 - cos / sqrt(sin^2 + cos^2)
    m["folded"] = (f32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -FOLD_COS, FOLD_SIN]]), i64([[0, 1, 2], [1, 0, 3]]))
    # three faces on the edge (0, 1): pairs (2,3), (2,4), (3,4); vertex 3 holds role 3 in one pair and role 2 in another
    m["three_on_edge"] = (f32([[0, 0, 0], [1, 0, 0], [0.25, 1, 0], [0.5, -0.5, 1], [0.75, -0.25, -1.5]]),
                          i64([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
    # unreferenced vertices: 4 at the origin, 5 elsewhere
    m["isolated"] = (f32([[1, 1, 1], [2, 1, 1], [1, 2, 1], [1, 1, 3], [0, 0, 0], [0.5, -2, 0.25]]),
                     i64([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
    m["flat_grid_5x5"] = tri_grid(5, 5)
    # face (0, 1, 4): vertex 4 sits on vertex 0, so its normal is exactly 0 and the edge (0, 4) has no length
    m["zero_normal"] = (f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.5, 1], [0, 0, 0]]),
                        i64([[0, 1, 2], [1, 0, 3], [0, 1, 4], [0, 4, 2]]))
    m["grid_15x17"] = tri_grid(15, 17, seed=1)            # V = 255
    m["grid_16x16"] = tri_grid(16, 16, seed=2)            # V = 256
    m["grid_16x16_plus_1"] = tri_grid(16, 16, 1, seed=3)  # V = 257
    return m
