"""TEST INFRASTRUCTURE ONLY: a numpy restatement of the distance fields (include/smilfit.h, "Distance fields").

``edt_brute`` is the definition itself - every (voxel, feature) pair, in int64.  ``sample_ref`` restates the sampler's rules in float64,
operation by operation, and returns float64 (the tests round once to float32, as the kernel does).
"""
import numpy as np

NONE = 2**31 - 1


def features(occ_frame, invert):
    """(F,3) int64 (i, j, k) of one frame's features; occ_frame is (Gz,Gy,Gx)."""
    k, j, i = np.nonzero((occ_frame == 0) if invert else (occ_frame != 0))
    return np.stack([i, j, k], axis=1).astype(np.int64)


def shell(G):
    """(S,3) int64: the one-voxel layer around a (Gx, Gy, Gz) grid - every index triple in [-1, G] with a coordinate equal to -1 or G."""
    Gx, Gy, Gz = G
    k, j, i = np.meshgrid(np.arange(-1, Gz + 1), np.arange(-1, Gy + 1), np.arange(-1, Gx + 1), indexing="ij")
    on = (i == -1) | (i == Gx) | (j == -1) | (j == Gy) | (k == -1) | (k == Gz)
    return np.stack([i[on], j[on], k[on]], axis=1).astype(np.int64)


def shell_distance(G):
    """(Gz,Gy,Gx) int64: min(i+1, Gx-i, j+1, Gy-j, k+1, Gz-k)^2, the squared distance to ``shell(G)`` (the nearest shell voxel lies straight
    along an axis; tests/test_distance_field_cpu.py checks this against the pairs)."""
    Gx, Gy, Gz = G
    i, j, k = np.arange(Gx, dtype=np.int64), np.arange(Gy, dtype=np.int64), np.arange(Gz, dtype=np.int64)
    d = np.minimum(np.minimum(np.minimum(i + 1, Gx - i)[None, None, :], np.minimum(j + 1, Gy - j)[None, :, None]), np.minimum(k + 1, Gz - k)[:, None, None])
    return d * d


def _frame(occ_frame, invert, border, shell_pairs, chunk=1 << 22):
    Gz, Gy, Gx = occ_frame.shape
    F = features(occ_frame, invert)
    if border and shell_pairs:
        F = np.concatenate([F, shell((Gx, Gy, Gz))])
    out = np.full((Gz, Gy, Gx), NONE, np.int64)
    if len(F):
        ax = [np.arange(g, dtype=np.int64) for g in (Gx, Gy, Gz)]
        step = max(1, chunk // (Gx * Gy * Gz))
        for f0 in range(0, len(F), step):
            f = F[f0:f0 + step]
            dx, dy, dz = ((ax[a][:, None] - f[None, :, a]) ** 2 for a in range(3))                 # (G_a, F)
            d = (dz[:, None, None, :] + dy[None, :, None, :] + dx[None, None, :, :]).min(axis=3)   # every pair
            out = np.minimum(out, d)
    if border and not shell_pairs:
        out = np.minimum(out, shell_distance((Gx, Gy, Gz)))
    return out


def edt_brute(occ, invert=False, border=False, shell_pairs=True):
    """d2 (N,Gz,Gy,Gx) int64 of occ (N,Gz,Gy,Gx): min over the features of the squared index distance; NONE where a frame has none.
    ``shell_pairs=False`` takes the border's shell through ``shell_distance`` instead of pair by pair (for grids whose shell is large)."""
    occ = np.asarray(occ)
    assert occ.ndim == 4
    return np.stack([_frame(o, bool(invert), bool(border), shell_pairs) for o in occ])


def _axis(p, origin, voxel, G):
    u = (p - origin) / voxel - 0.5
    c = np.clip(u, 0.0, float(G - 1))
    i0 = np.zeros(p.shape, np.int64) if G == 1 else np.minimum(np.floor(c).astype(np.int64), G - 2)
    i1 = np.minimum(i0 + 1, G - 1)
    out = u - c
    return i0, i1, c - i0, out, (out == 0.0) & (G > 1)


def _lerp(a, b, t):
    return (1.0 - t) * a + t * b


def sample_ref(d2_out, d2_in, origin, voxel, points, point_dim):
    """``(value (N,P), grad (N,P,point_dim))`` float64.  d2_out / d2_in (None): (N,Gz,Gy,Gx) integers; origin (1 or N,3), voxel (1 or N) float64;
    points (N,P,point_dim) float32 ((y, x) for point_dim 2, which needs Gz = 1)."""
    d2_out = np.asarray(d2_out)
    N, Gz, Gy, Gx = d2_out.shape
    origin = np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 3), (N, 3))
    voxel = np.broadcast_to(np.asarray(voxel, np.float64).reshape(-1), (N,))
    pts = np.asarray(points)
    assert pts.dtype == np.float32 and pts.shape[0] == N and pts.shape[2] == point_dim and (point_dim == 3 or Gz == 1)
    pts = pts.astype(np.float64)
    r = np.sqrt(d2_out.astype(np.float64))
    if d2_in is not None:
        d2_in = np.asarray(d2_in)
        r = r - np.where(d2_in == NONE, 0.0, np.sqrt(d2_in.astype(np.float64)))
    r = np.where(d2_out == NONE, 0.0, r)  # no hull in the frame: no field
    xyz = pts[..., ::-1] if point_dim == 2 else pts  # (x, y[, z])
    finite = np.isfinite(pts).all(axis=2)
    safe = np.where(finite[..., None], xyz, 0.0)
    vox = voxel[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        X = _axis(safe[..., 0], origin[:, 0:1], vox, Gx)
        Y = _axis(safe[..., 1], origin[:, 1:2], vox, Gy)
        if point_dim == 3:
            Z = _axis(safe[..., 2], origin[:, 2:3], vox, Gz)
        else:
            z = np.zeros(finite.shape)
            Z = (z.astype(np.int64), z.astype(np.int64), z, z, z.astype(bool))
        n = np.arange(N)[:, None]
        c = [[[r[n, (Z[1] if k else Z[0]), (Y[1] if j else Y[0]), (X[1] if i else X[0])] for i in (0, 1)] for j in (0, 1)] for k in (0, 1)]
        v, dx, dy = [], [], []
        for k in (0, 1):
            a0, a1 = _lerp(c[k][0][0], c[k][0][1], X[2]), _lerp(c[k][1][0], c[k][1][1], X[2])
            v.append(_lerp(a0, a1, Y[2]))
            dx.append(_lerp(c[k][0][1] - c[k][0][0], c[k][1][1] - c[k][1][0], Y[2]))
            dy.append(a1 - a0)
        dist = np.sqrt(X[3] * X[3] + Y[3] * Y[3] + Z[3] * Z[3])
        value = vox * (_lerp(v[0], v[1], Z[2]) + dist)
        g = [np.where(X[4], _lerp(dx[0], dx[1], Z[2]), 0.0), np.where(Y[4], _lerp(dy[0], dy[1], Z[2]), 0.0), np.where(Z[4], v[1] - v[0], 0.0)]
        away = dist > 0.0
        g = [gi + np.where(away, A[3] / np.where(away, dist, 1.0), 0.0) for gi, A in zip(g, (X, Y, Z))]
    value = np.where(finite, value, 0.0)
    g = [np.where(finite, gi, 0.0) for gi in g]
    grad = np.stack([g[1], g[0]] if point_dim == 2 else g, axis=2)
    return value, grad
