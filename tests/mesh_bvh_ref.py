"""A numpy restatement of the mesh hierarchy of smilify_amd/csrc/mesh_bvh.hip, for tests: the implicit heap over Morton-sorted faces,
the exact boxes, and the traversal's rules - nearer child first, the key {d^2, face} compared lexicographically, a node entered
when D^2 <= (sqrt(best) + EPS)^2 (1 + 2^-19).  It is slow and runs anywhere.  One mesh at a time.

The leaf distances are tests/point_mesh_ref.py's formula evaluated in float32 on the frame's coordinates: equal to the kernel's on
inputs whose products are exact (the tie cases), not in general - the GPU tests compare kernel with kernel."""
import numpy as np
import torch

import point_mesh_ref as PR

EPS = np.float32(2.0 ** -18)
SLACK = np.float32(1.0 + 2.0 ** -19)
SENTINEL = 1 << 30
INF = np.float32(np.inf)


def usable_faces(verts, faces):
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < len(v))).all(1)
    tri = v[np.clip(f, 0, max(len(v) - 1, 0))] if len(v) else np.zeros((len(f), 3, 3), np.float32)
    with np.errstate(invalid="ignore"):
        return inside & (np.abs(tri) <= PR.USABLE).all((1, 2)), tri


def _spread10(x):
    x = x & 0x3FF
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def morton(p, lo, hi):
    """30-bit codes of points p (n,3) inside lo .. hi, 10 bits an axis, z the most significant (float32 as the kernel)."""
    p, lo, hi = (np.asarray(t, np.float32) for t in (p, lo, hi))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.float32(0.5) * p - np.float32(0.5) * lo) / (np.float32(0.5) * hi - np.float32(0.5) * lo)
    t = np.where(t > 0, np.minimum(t, np.float32(1)), np.float32(0))  # NaN -> 0
    q = (t * np.float32(1023)).astype(np.int64)
    return _spread10(q[:, 0]) | (_spread10(q[:, 1]) << 1) | (_spread10(q[:, 2]) << 2)


def boxes_of(verts, faces, order, leaf):
    """(L, Lp, boxes (2 Lp, 6)): heap rows 1 .. 2 Lp - 1, lo xyz and hi xyz, empty = +inf .. -inf."""
    ok, tri = usable_faces(verts, faces)
    F = len(tri)
    L = -(-F // leaf)
    Lp = 1 << max(L - 1, 0).bit_length()
    boxes = np.empty((2 * Lp, 6), np.float32)
    boxes[:, :3], boxes[:, 3:] = np.inf, -np.inf
    for k in range(L):
        ids = [j for j in order[k * leaf:(k + 1) * leaf] if 0 <= j < F and ok[j]]
        if ids:
            boxes[Lp + k, :3], boxes[Lp + k, 3:] = tri[ids].min((0, 1)), tri[ids].max((0, 1))
    for i in range(Lp - 1, 0, -1):
        boxes[i, :3], boxes[i, 3:] = np.minimum(boxes[2 * i, :3], boxes[2 * i + 1, :3]), np.maximum(boxes[2 * i, 3:], boxes[2 * i + 1, 3:])
    return L, Lp, boxes


def build(verts, faces, leaf):
    """dict(order, L, Lp, boxes, leaf) of one mesh: the stable sort of the faces' codes, unusable faces behind the rest."""
    ok, tri = usable_faces(verts, faces)
    codes = np.full(len(tri), SENTINEL, np.int64)
    if ok.any():
        lo, hi = tri[ok].min((0, 1)), tri[ok].max((0, 1))
        third = np.float32(1.0 / 3.0)
        mid = tri[ok][:, 0] * third + tri[ok][:, 1] * third + tri[ok][:, 2] * third
        codes[ok] = morton(mid, lo, hi)
    order = np.argsort(codes, kind="stable")
    L, Lp, boxes = boxes_of(verts, faces, order, leaf)
    return dict(order=order, L=L, Lp=Lp, boxes=boxes, leaf=leaf)


def frame_shift(verts, faces, points):
    """sh of the search's frame: coordinates times 2^sh lie below 1 (k_pm_extent: faces with indices in range, finite coordinates)."""
    v, f, p = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(points, np.float32)
    inside = ((f >= 0) & (f < len(v))).all(1)
    vals = np.concatenate([np.abs(v[f[inside]]).ravel(), np.abs(p).ravel(), [0.0]])
    with np.errstate(invalid="ignore"):
        big = np.float32(vals[vals <= PR.USABLE].max())
    return -int(np.frexp(big)[1])


def pair_table(verts, faces, points, sh):
    """d^2 (P, F) float32 of every pair in the frame, NaN where the face or the point is not usable."""
    ok, tri = usable_faces(verts, faces)
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p_ok = (np.abs(p) <= PR.USABLE).all(1)
        t32 = torch.from_numpy(np.ldexp(np.where(ok[:, None, None], tri, 0), sh).astype(np.float32))
        p32 = torch.from_numpy(np.ldexp(np.where(p_ok[:, None], p, 0), sh).astype(np.float32))
    d = PR.closest_on_triangle(p32[:, None, :], t32[None])[1].numpy().astype(np.float32)
    d[~p_ok, :] = np.nan
    d[:, ~ok] = np.nan
    return d


def _box_d2(row, sh, p):
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.ldexp(row[:3], sh).astype(np.float32), np.ldexp(row[3:], sh).astype(np.float32)
        d = np.maximum(np.maximum(lo - p, p - hi), np.float32(0))
        return np.float32((d * d).sum(dtype=np.float32))


def _limit(best):
    s = np.float32(np.sqrt(best, dtype=np.float32) + EPS)
    return np.float32(np.float32(s * s) * SLACK)


def query(tree, verts, faces, points, margin: bool = True, tie_rule: bool = True):
    """(d^2 in the frame (P) float32, face (P) int64 or -1, evaluated (P)) by the traversal of k_bvh_points.  `margin` False: EPS = 0
    and no slack; `tie_rule` False: a node is entered only when D^2 < the limit - the two ways to be wrong, for the tests."""
    sh = frame_shift(verts, faces, points)
    table = pair_table(verts, faces, points, sh)
    order, Lp, boxes, leaf, F = tree["order"], tree["Lp"], tree["boxes"], tree["leaf"], len(tree["order"])
    D = Lp.bit_length() - 1
    limit_of = _limit if margin else (lambda b: np.float32(b))
    enter = (lambda d, lim: d <= lim and d < INF) if tie_rule else (lambda d, lim: d < lim or (lim == INF and d < INF))
    out_d, out_f, out_n = np.full(len(table), INF, np.float32), np.full(len(table), -1, np.int64), np.zeros(len(table), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        p_ok = (np.abs(np.asarray(points, np.float32)) <= PR.USABLE).all(1)
        pf = np.ldexp(np.asarray(points, np.float32), sh).astype(np.float32)
    for q in range(len(table)):
        if F == 0 or not p_ok[q]:  # (nothing wins for an unusable point, and no box distance means anything)
            continue
        best, bi, limit, count = INF, 0x7FFFFFFF, INF, 0
        i, owed, down = 1, 0, True
        while True:
            if down:
                level = i.bit_length() - 1
                if level == D:
                    s0 = (i - Lp) * leaf
                    for s in range(s0, min(F, s0 + leaf)):
                        d, f = table[q, order[s]], int(order[s])
                        if d < best or (d == best and f < bi):
                            best, bi = d, f
                        count += 1
                    limit, down = limit_of(best), False
                else:
                    d0, d1 = _box_d2(boxes[2 * i], sh, pf[q]), _box_d2(boxes[2 * i + 1], sh, pf[q])
                    in0, in1 = enter(d0, limit), enter(d1, limit)
                    if in0 or in1:
                        if in0 and in1:
                            owed |= 1 << (level + 1)
                        i = 2 * i + (1 if in1 and (not in0 or d1 < d0) else 0)
                    else:
                        down = False
            else:
                if owed == 0:
                    break
                lv = owed.bit_length() - 1
                owed &= ~(1 << lv)
                i = (i >> ((i.bit_length() - 1) - lv)) ^ 1
                down = bool(enter(_box_d2(boxes[i], sh, pf[q]), limit))
        if best < INF:
            out_d[q], out_f[q] = best, bi
        out_n[q] = count
    return out_d, out_f, out_n


def brute(verts, faces, points):
    """(d^2 in the frame (P) float32, face (P)) by the sequential scan with a strict <: what the traversal must reproduce."""
    table = pair_table(verts, faces, points, frame_shift(verts, faces, points))
    out_d, out_f = np.full(len(table), INF, np.float32), np.full(len(table), -1, np.int64)
    for q, row in enumerate(table):
        live = ~np.isnan(row)
        if live.any():
            out_d[q] = row[live].min()
            out_f[q] = int(np.nonzero(live & (row == out_d[q]))[0][0])
    return out_d, out_f
