"""TEST INFRASTRUCTURE ONLY: the visual hull of ``smilify_amd/csrc/visual_hull.hip`` restated in numpy float64 from the header comment of
``include/smilfit.h`` ("Visual hull").  Holds no kernels and touches no GPU.

Camera arithmetic (that of smil_kp2d_fit_eval, float64 on the float32 tables): ``X_view = X R + T``; ``k11 = 1 / tan(fov / 2)``, ``k00 = k11 /
aspect``; ``x_ndc = k00 x / z + px``; ``y_s = S/2 - (S/2) y_ndc``, ``x_s`` likewise.  Image ``n * Nv + v``; a table with k rows (1, Nv or N * Nv) is
indexed ``image % k``.  ``cams``: dict with ``R (k,3,3)``, ``T (k,3)``, ``fov (k,)`` degrees and optionally ``aspect_ratio (k,)`` and
``principal_point (k,2)`` - the dict ``visual_hull.carve`` takes.  A view sees a point iff ``z > ZNEAR``, ``0 <= y_s < H`` and ``0 <= x_s < W``;
a seen point is foreground iff ``mask[floor(y_s), floor(x_s)] > threshold``.

The GPU's float64 differs from numpy's in ``tan``, the division and contraction by parts in 1e-13, so a (point, view) pair whose decision
hangs on less than that cannot be pinned.  ``votes`` therefore also returns, per pair, an AMBIGUOUS flag - ``|y_s - round(y_s)| < 1e-7``, or
the same for ``x_s``, or ``|z_view - ZNEAR| < 1e-9`` - and derives per-point lower and upper bounds of ``fg`` and ``seen`` from it: an
ambiguous pair may or may not count.  Where the bounds coincide the counts are exact.
"""
import numpy as np

ZNEAR = float(np.float32(0.001))  # SMIL_ZNEAR as the kernels hold it
EDGE_MARGIN = 1e-7
Z_MARGIN = 1e-9


def _rows(t, tail, n_img):
    t = np.asarray(t, np.float32).reshape(-1, *tail)  # the library holds float32 tables
    return t[np.arange(n_img) % t.shape[0]].astype(np.float64)


def camera_tables(cams, N, views):
    """The per-image float64 tables (R (n,3,3), T (n,3), k00 (n,), k11 (n,), pp (n,2)) of N * views images."""
    n_img = N * views
    R, T = _rows(cams["R"], (3, 3), n_img), _rows(cams["T"], (3,), n_img)
    fov = _rows(cams["fov"], (), n_img)
    k11 = 1.0 / np.tan(fov * 0.017453292519943295 / 2.0)
    k00 = k11 / _rows(cams["aspect_ratio"], (), n_img) if cams.get("aspect_ratio") is not None else k11.copy()
    pp = _rows(cams["principal_point"], (2,), n_img) if cams.get("principal_point") is not None else np.zeros((n_img, 2))
    return R, T, k00, k11, pp


def project(points, cams, S, views):
    """points (N,P,3) -> (y_s, x_s, z_view), each (N,Nv,P) float64."""
    points = np.asarray(points, np.float64)
    N, P = points.shape[:2]
    R, T, k00, k11, pp = (t.reshape(N, views, *t.shape[1:]) for t in camera_tables(cams, N, views))
    X, Y, Z = (points[:, None, :, k] for k in range(3))
    r = lambda a, b: R[:, :, a, b][:, :, None]  # noqa: E731
    vx = X * r(0, 0) + Y * r(1, 0) + Z * r(2, 0) + T[:, :, 0, None]
    vy = X * r(0, 1) + Y * r(1, 1) + Z * r(2, 1) + T[:, :, 1, None]
    vz = X * r(0, 2) + Y * r(1, 2) + Z * r(2, 2) + T[:, :, 2, None]
    with np.errstate(all="ignore"):
        iz = 1.0 / vz
        xn, yn = vx * k00[:, :, None] * iz, vy * k11[:, :, None] * iz
        hS = 0.5 * float(S)
        ys, xs = hS - hS * (yn + pp[:, :, 1, None]), hS - hS * (xn + pp[:, :, 0, None])
    return ys, xs, vz


class Votes:
    """fg, seen (N,P) int: the counts as numpy decides them; *_lo / *_hi their bounds; ambiguous (N,Nv,P) bool."""


def votes(points, masks, cams, S, threshold=0.0, outside_carves=False):
    masks = np.asarray(masks)
    N, views, H, W = masks.shape
    ys, xs, z = project(points, cams, S, views)
    with np.errstate(invalid="ignore"):
        front = z > ZNEAR
        inside = front & (ys >= 0.0) & (ys < H) & (xs >= 0.0) & (xs < W)
        amb_z = np.abs(z - ZNEAR) < Z_MARGIN
        amb_xy = (np.abs(ys - np.round(ys)) < EDGE_MARGIN) | (np.abs(xs - np.round(xs)) < EDGE_MARGIN)
    r = np.where(inside, np.floor(np.where(inside, ys, 0.0)), 0).astype(np.int64)
    c = np.where(inside, np.floor(np.where(inside, xs, 0.0)), 0).astype(np.int64)
    n_i, v_i = np.arange(N)[:, None, None], np.arange(views)[None, :, None]
    with np.errstate(invalid="ignore"):
        value = masks[n_i, v_i, r, c].astype(np.float32) > np.float32(threshold)  # (a NaN is not)
    fg_pair = inside & value
    seen_pair = front if outside_carves else inside
    amb_fg = amb_z | amb_xy
    amb_seen = amb_z if outside_carves else amb_fg
    out = Votes()
    out.fg, out.seen = fg_pair.sum(1), seen_pair.sum(1)
    out.fg_lo, out.fg_hi = (fg_pair & ~amb_fg).sum(1), (fg_pair | amb_fg).sum(1)
    out.seen_lo, out.seen_hi = (seen_pair & ~amb_seen).sum(1), (seen_pair | amb_seen).sum(1)
    out.ambiguous = amb_fg
    out.exact = (out.fg_lo == out.fg_hi) & (out.seen_lo == out.seen_hi)  # (N,P): no ambiguous pair touches the point
    return out


def occupancy_rule(fg, seen, min_views, max_misses):
    return ((seen >= min_views) & (seen - fg <= max_misses)).astype(np.uint8)


def grid_tables(N, origin, voxel_size):
    origin = np.asarray(origin, np.float64).reshape(-1, 3)
    voxel = np.asarray(voxel_size, np.float64).reshape(-1)
    return origin[np.arange(N) % origin.shape[0]], voxel[np.arange(N) % voxel.shape[0]]


def centres(N, origin, voxel_size, grid):
    """(N, Gz*Gy*Gx, 3) float64 voxel centres in linear index order (x fastest): origin + (index + 0.5) * voxel_size, a product and a sum."""
    Gx, Gy, Gz = grid
    origin, voxel = grid_tables(N, origin, voxel_size)
    k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    idx = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64)
    return origin[:, None, :] + (idx[None] + 0.5) * voxel[:, None, None]


def points_at(linear, frame, origin, voxel_size, grid):
    """Centres (float64) of the voxels with the given linear indices of the given frames (both (M,))."""
    Gx, Gy, _ = grid
    linear = np.asarray(linear, np.int64)
    idx = np.stack([linear % Gx, (linear // Gx) % Gy, linear // (Gx * Gy)], axis=1).astype(np.float64)
    origin = np.asarray(origin, np.float64).reshape(-1, 3)
    voxel = np.asarray(voxel_size, np.float64).reshape(-1)
    frame = np.asarray(frame, np.int64)
    return origin[frame % origin.shape[0]] + (idx + 0.5) * voxel[frame % voxel.shape[0]][:, None]


def carve(masks, cams, S, origin, voxel_size, grid, min_views=2, max_misses=0, outside_carves=False, threshold=0.0):
    """-> (occ (N,Gz,Gy,Gx) uint8, votes): ``votes`` of the voxel centres with every (N,P) array reshaped to the grid."""
    N = np.asarray(masks).shape[0]
    Gx, Gy, Gz = grid
    v = votes(centres(N, origin, voxel_size, grid), masks, cams, S, threshold, outside_carves)
    for name in ("fg", "seen", "fg_lo", "fg_hi", "seen_lo", "seen_hi", "exact"):
        setattr(v, name, getattr(v, name).reshape(N, Gz, Gy, Gx))
    return occupancy_rule(v.fg, v.seen, min_views, max_misses), v


def stats(occ):
    """(N,16) int64 of occ (N,Gz,Gy,Gx): count; sums of i, j, k; of i^2, j^2, k^2, ij, ik, jk; minima and maxima of i, j, k (an empty frame
    keeps Gx, Gy, Gz and -1)."""
    N, Gz, Gy, Gx = occ.shape
    out = np.zeros((N, 16), np.int64)
    for n in range(N):
        k, j, i = (a.astype(np.int64) for a in np.nonzero(occ[n]))
        out[n, :10] = [i.size, i.sum(), j.sum(), k.sum(), (i * i).sum(), (j * j).sum(), (k * k).sum(), (i * j).sum(), (i * k).sum(), (j * k).sum()]
        out[n, 10:13] = [i.min(), j.min(), k.min()] if i.size else [Gx, Gy, Gz]
        out[n, 13:16] = [i.max(), j.max(), k.max()] if i.size else [-1, -1, -1]
    return out


def moments(st, origin, voxel_size):
    """count (N,), centroid (N,3), covariance (N,3,3) float64 from the integer sums (NaN rows for an empty frame)."""
    st = np.asarray(st)
    N = st.shape[0]
    origin, voxel = grid_tables(N, origin, voxel_size)
    with np.errstate(all="ignore"):
        n = st[:, 0].astype(np.float64)
        mean = st[:, 1:4] / n[:, None]
        second = np.empty((N, 3, 3))
        for (a, b), col in (((0, 0), 4), ((1, 1), 5), ((2, 2), 6), ((0, 1), 7), ((0, 2), 8), ((1, 2), 9)):
            second[:, a, b] = second[:, b, a] = st[:, col] / n
        cov = (second - mean[:, :, None] * mean[:, None, :]) * (voxel * voxel)[:, None, None]
    return st[:, 0], origin + (mean + 0.5) * voxel[:, None], cov


def surface(occ, origin, voxel_size):
    """-> (points (total,3) float32, index (total,) int64, offsets (N+1,) int64): the occupied voxels with an unoccupied 6-neighbour (the
    border counts as unoccupied), frames in order, ascending linear index within a frame; centres in float64, rounded once."""
    N, Gz, Gy, Gx = occ.shape
    origin, voxel = grid_tables(N, origin, voxel_size)
    o = np.pad(occ != 0, ((0, 0), (1, 1), (1, 1), (1, 1)))
    c = o[:, 1:-1, 1:-1, 1:-1]
    inner = (o[:, 1:-1, 1:-1, :-2] & o[:, 1:-1, 1:-1, 2:] & o[:, 1:-1, :-2, 1:-1] & o[:, 1:-1, 2:, 1:-1] & o[:, :-2, 1:-1, 1:-1] &
             o[:, 2:, 1:-1, 1:-1])
    surf = c & ~inner
    pts, idx, offsets = [], [], [0]
    for n in range(N):
        lin = np.flatnonzero(surf[n].ravel()).astype(np.int64)
        ijk = np.stack([lin % Gx, (lin // Gx) % Gy, lin // (Gx * Gy)], axis=1).astype(np.float64)
        pts.append((origin[n] + (ijk + 0.5) * voxel[n]).astype(np.float32))
        idx.append(lin)
        offsets.append(offsets[-1] + lin.size)
    return np.concatenate(pts).reshape(-1, 3), np.concatenate(idx), np.asarray(offsets, np.int64)
