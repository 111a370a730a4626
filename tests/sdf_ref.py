"""Float64 CPU restatement of the SDF-guided registration term (reference fitter_3d/utils.py:973-1394):

* ``knn_brute``: the K nearest candidates of every query by brute force, rows ordered by ``np.argsort(kind="stable")`` on the float64
  squared distances, which is exactly ascending (distance, index);
* ``sdf_term_at``: the term at given neighbour indices in any torch dtype: z-scores per (mesh, side) with the unbiased std clamped at
  1e-8, softmax over the K neighbours of -|z_q - z_c| / 0.1, the weighted sum of the squared distances, point and batch reduction,
  both directions added.  In float64 it is the reference value (and autograd its gradient), in float32 the yardstick of what plain
  torch ops reach on the same indices;
* ``sdf_grad_at``: the analytic gradient at given indices (only the distances carry one);
* ``vertex_indices``: the vertex sampler's index draw, restated with exact integers.

tests/golden/sdf_distance_ref.npz holds the reference's own SDF_distance on small inputs; tests/test_sdf_cpu.py compares.
"""
import numpy as np
import torch

from mesh3d_ref import philox4x32_10

TEMPERATURE = 0.1
STD_MIN = 1e-8
SV_STREAM = 1  # third Philox counter word of the vertex sampler (the surface sampler uses 0)


def knn_brute(q, c, K, chunk=128):
    """q (N,Pq,3), c (N,Pc,3) -> (dists (N,Pq,K) float64, idx (N,Pq,K) int64, the (K+1)-th distance (N,Pq), inf when K = Pc)."""
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    N, Pq, Pc = q.shape[0], q.shape[1], c.shape[1]
    dists, idx, nxt = np.empty((N, Pq, K)), np.empty((N, Pq, K), np.int64), np.full((N, Pq), np.inf)
    for n in range(N):
        for i in range(0, Pq, chunk):
            d = ((q[n, i:i + chunk, None, :] - c[n][None, :, :]) ** 2).sum(-1)
            o = np.argsort(d, axis=1, kind="stable")
            idx[n, i:i + chunk] = o[:, :K]
            ds = np.take_along_axis(d, o, 1)
            dists[n, i:i + chunk] = ds[:, :K]
            if K < Pc:
                nxt[n, i:i + chunk] = ds[:, K]
    return dists, idx, nxt


def _zscore(s):
    return (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True).clamp(min=STD_MIN)


def _direction(q, c, zq, zc, idx, point_sum, batch_sum):
    N, Pq, K = idx.shape
    flat = idx.reshape(N, Pq * K)
    cj = torch.gather(c, 1, flat[..., None].expand(-1, -1, 3)).reshape(N, Pq, K, 3)
    d = ((q[:, :, None, :] - cj) ** 2).sum(-1)
    w = torch.softmax(-(zq[:, :, None] - torch.gather(zc, 1, flat).reshape(N, Pq, K)).abs() / TEMPERATURE, dim=-1)
    r = (w * d).sum(-1)
    per = r.sum(1) if point_sum else r.mean(1)
    return per.sum() if batch_sum else per.mean()


def sdf_term_at(x, y, xs, ys, ix, iy, point_sum=False, batch_sum=False, single_directional=False):
    """The term of torch tensors x (N,P1,3), y (N,P2,3), xs (N,P1), ys (N,P2) at the indices ix (N,P1,K), iy (N,P2,K) int64."""
    zx, zy = _zscore(xs), _zscore(ys)
    loss = _direction(x, y, zx, zy, ix, point_sum, batch_sum)
    if not single_directional:
        loss = loss + _direction(y, x, zy, zx, iy, point_sum, batch_sum)
    return loss


def sdf_term(x, y, xs, ys, K, point_sum=False, batch_sum=False, single_directional=False, dtype=torch.float64, with_grad=False):
    """Brute-force search, then the term in ``dtype``: (loss, ix, iy) or, with_grad, (loss, d_x, d_y, ix, iy) as numpy float64."""
    _, ix, _ = knn_brute(x, y, K)
    iy = None if single_directional else knn_brute(y, x, K)[1]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    ti = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    X, Y = t(x).requires_grad_(with_grad), t(y).requires_grad_(with_grad)
    loss = sdf_term_at(X, Y, t(xs), t(ys), ti(ix), ti(iy), point_sum, batch_sum, single_directional)
    if not with_grad:
        return float(loss), ix, iy
    gx, gy = torch.autograd.grad(loss, (X, Y), allow_unused=True)
    gy = torch.zeros_like(Y) if gy is None else gy
    return float(loss.detach()), gx.double().numpy(), gy.double().numpy(), ix, iy


def sdf_grad_at(x, y, xs, ys, ix, iy, point_sum=False, batch_sum=False, single_directional=False):
    """The analytic float64 gradient at the given indices: dr_i/dq_i = sum_k 2 w_ik (q_i - c_j), its negative scattered to c_j."""
    x, y, xs, ys = (np.asarray(a, np.float64) for a in (x, y, xs, ys))
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    z = lambda s: (s - s.mean(1, keepdims=True)) / np.maximum(s.std(1, ddof=1, keepdims=True), STD_MIN)  # noqa: E731
    zx, zy = z(xs), z(ys)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    bw = 1.0 if batch_sum else 1.0 / N

    def one(q, c, zq, zc, idx, gq, gc, wq):
        for n in range(N):
            a = -np.abs(zq[n][:, None] - zc[n][idx[n]]) / TEMPERATURE
            w = np.exp(a - a.max(1, keepdims=True))
            w /= w.sum(1, keepdims=True)
            e = 2.0 * wq * w[..., None] * (q[n][:, None, :] - c[n][idx[n]])
            gq[n] += e.sum(1)
            np.add.at(gc[n], idx[n].reshape(-1), -e.reshape(-1, 3))

    one(x, y, zx, zy, ix, gx, gy, (1.0 if point_sum else 1.0 / P1) * bw)
    if not single_directional:
        one(y, x, zy, zx, iy, gy, gx, (1.0 if point_sum else 1.0 / P2) * bw)
    return gx, gy


def vertex_index(r, V):
    """The sampler's map of a 32-bit draw r to a vertex of a mesh of V vertices: (r * V) >> 32, in exact integers."""
    return (int(r) * int(V)) >> 32


def vertex_indices(n, S, seed, V):
    """The vertex of samples 0 .. S-1 of mesh n: word 0 of Philox4x32-10 at counter (s, n, 1, 0) under the key (seed lo, seed hi)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((np.arange(S, dtype=np.uint64), np.full(S, n, np.uint64), SV_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return np.array([vertex_index(v, V) for v in r.tolist()], np.int64)
