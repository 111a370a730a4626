"""Float64 restatement of the spatial-diameter ray cast (reference fitter_3d/SDF_tests.py:112-222, 344-382) and of its two
K-nearest steps (:387-415, :775-818), with a classification of the rays a float32 evaluation may legitimately decide differently.

* ``cast``: per ray and face, with e1 = v1 - v0, e2 = v2 - v0, h = d x e2, a = e1 . h, f = 1 / a, s = o - v0, u = f (s . h),
  q = s x e1, v = f (d . q), t = f (e2 . q): face j is hit when j != own_face, |a| > 1e-6, 0 <= u <= 1, v >= 0, u + v <= 1 and
  t > t_min.  The ray's value is the LARGEST t over its hits (-1: none).
* ``diameters``: per sample, rays in order; a ray is valid when it has a hit with d_lo < t < d_hi; the walk stops once ``cap`` valid
  rays are taken; the mean of those, or d_lo.
* ambiguity: a face is undecided when it passes every test relaxed by m and fails some test tightened by m, where
  m = max(1e-4, 16 * 2^-24 |s||h| / |a|) (the forward error of the dot product over a) is absolute on u, v, u + v and relative on
  |a| against 1e-6 and on t against t_min.  A ray is ambiguous when an undecided face could change its maximum (its t exceeds the
  largest t of the decided hits), when its maximum lies within relative m of d_lo or d_hi, or when the float32 error bound of its
  winning face's t, 16 * 2^-24 (|t| + |e2||q| / |a|), exceeds 1e-5 of the bounding-box diagonal.
* ``smooth`` / ``vertex_values``: the mean over the k nearest points, and the inverse-distance weighted, min-max scaled vertex values,
  from a brute-force search ordered by (distance, index); both also return which rows' neighbour sets are determined (the k-th and
  (k+1)-th distances differ by more than float32 rounding of the squared distances).
"""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN, MODEL_FILES
from sdf_ref import knn_brute

U = 2.0 ** -24
EPS_A = 1e-6
M_MIN = 1e-4


def thresholds(verts):
    """(diag, d_lo, d_hi, offset) as compute_sdf forms them: float32 products of the float32 diagonal."""
    v = np.asarray(verts, np.float32)
    diag = np.float32(np.sqrt(np.sum((v.max(0) - v.min(0)).astype(np.float32) ** 2, dtype=np.float32)))
    return diag, np.float32(diag * np.float32(0.001)), np.float32(diag * np.float32(0.2)), np.float32(diag * np.float32(0.0001))


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def cast(verts, faces, origins, own_face, dirs, t_min, d_lo=None, d_hi=None, diag=None, chunk_bytes=64 << 20):
    """verts (V,3), faces (F,3), origins (S,3), own_face (S), dirs (S,R,3) -> dict of (S,R) arrays: ``t`` the largest hit distance
    (-1: none), ``face`` its face (-1; the smallest index among equal t), ``bound`` the float32 error bound of t, and, when d_lo, d_hi
    and diag are given, ``ambiguous``.

    Two passes, the same arithmetic throughout: h, a, u and m for every (ray, face); then v, t and the tests only where the relaxed
    test on u and |a| holds, which every hit, relaxed and tightened pass implies."""
    verts, origins, dirs = (np.ascontiguousarray(np.asarray(x, np.float64)) for x in (verts, origins, dirs))
    faces, own_face = np.asarray(faces, np.int64), np.asarray(own_face, np.int64)
    S, R, F = dirs.shape[0], dirs.shape[1], faces.shape[0]
    v0 = verts[faces[:, 0]]
    e1, e2 = verts[faces[:, 1]] - v0, verts[faces[:, 2]] - v0
    e2n = np.linalg.norm(e2, axis=1)
    classify = d_lo is not None
    t_out, face_out, bound_out, amb_out = np.full(S * R, -1.0), np.full(S * R, -1, np.int64), np.zeros(S * R), np.zeros(S * R, bool)
    step = max(1, int(chunk_bytes // (R * F * 8 * 14)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s0 in range(0, S, step):
            s1 = min(S, s0 + step)
            d = dirs[s0:s1]
            sv = origins[s0:s1, None, :] - v0[None]                               # (s, F, 3)
            # the dense pass runs on torch's float64 CPU kernels (the same IEEE operations as numpy's, on several threads)
            T = torch.from_numpy
            dx, dy, dz = (T(d[:, :, k, None]) for k in range(3))                  # (s, R, 1)
            hx, hy, hz = _cross(dx, dy, dz, T(e2[:, 0]), T(e2[:, 1]), T(e2[:, 2]))  # (s, R, F)
            a = T(e1[:, 0]) * hx + T(e1[:, 1]) * hy + T(e1[:, 2]) * hz
            sx, sy, sz = (T(sv[:, None, :, k]) for k in range(3))                 # (s, 1, F)
            f = 1.0 / a
            u = f * (sx * hx + sy * hy + sz * hz)
            m = 16 * U * torch.sqrt(sx * sx + sy * sy + sz * sz) * torch.sqrt(hx * hx + hy * hy + hz * hz) / a.abs()
            m = torch.where(m >= M_MIN, m, torch.full_like(m, M_MIN))             # (NaN from a = 0: M_MIN; such faces fail |a| > 0)
            cand = (a.abs() > 0) & (a.abs() > EPS_A * (1 - m)) & (u >= -m) & (u <= 1 + m)
            cand &= T(np.arange(F)[None, :] != own_face[s0:s1, None])[:, None, :]
            si, ri, fi = (x.numpy() for x in torch.nonzero(cand, as_tuple=True))
            a, f, u, m = (x.numpy()[si, ri, fi] for x in (a, f, u, m))
            rid = (s0 + si) * R + ri
            dc, svc, e1c, e2c = d[si, ri], sv[si, fi], e1[fi], e2[fi]
            qx, qy, qz = _cross(svc[:, 0], svc[:, 1], svc[:, 2], e1c[:, 0], e1c[:, 1], e1c[:, 2])
            v = f * (dc[:, 0] * qx + dc[:, 1] * qy + dc[:, 2] * qz)
            t = f * (e2c[:, 0] * qx + e2c[:, 1] * qy + e2c[:, 2] * qz)
            hit = (np.abs(a) > EPS_A) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > t_min)
            bound = 16 * U * (np.abs(t) + e2n[fi] * np.sqrt(qx * qx + qy * qy + qz * qz) / np.abs(a))
            tmax = np.full(S * R, -np.inf)
            np.maximum.at(tmax, rid[hit], t[hit])
            got = np.isfinite(tmax)
            t_out[got] = tmax[got]
            w = np.nonzero(hit & (t == tmax[rid]))[0][::-1]                       # (reversed: the smallest face index is written last)
            face_out[rid[w]], bound_out[rid[w]] = fi[w], bound[w]
            if not classify:
                continue
            relaxed = (v >= -m) & (u + v <= 1 + m) & (t > t_min * (1 - m))        # (|a| and u: relaxed already)
            tight = (np.abs(a) > EPS_A * (1 + m)) & (u >= m) & (u <= 1 - m) & (v >= m) & (u + v <= 1 - m) & (t > t_min * (1 + m))
            t_decided = np.full(S * R, -np.inf)
            np.maximum.at(t_decided, rid[tight], t[tight])
            amb_out[rid[relaxed & ~tight & (t > t_decided[rid])]] = True
            mw = np.zeros(S * R)
            mw[rid[w]] = m[w]
            near = got & ((np.abs(tmax - d_lo) <= mw * d_lo) | (np.abs(tmax - d_hi) <= mw * d_hi))
            amb_out |= near | (got & (bound_out > 1e-5 * float(diag)))
    return dict(t=t_out.reshape(S, R), face=face_out.reshape(S, R), bound=bound_out.reshape(S, R), ambiguous=amb_out.reshape(S, R))


def diameters(ray_t, d_lo, d_hi, cap):
    """ray_t (S,R) (-1: no hit) -> (S,) float64: the mean of the first ``cap`` valid rays of every sample in ray order, or d_lo."""
    ray_t = np.asarray(ray_t, np.float64)
    out = np.empty(ray_t.shape[0])
    for s, row in enumerate(ray_t):
        ok = row[(row >= 0) & (row > d_lo) & (row < d_hi)][:cap]
        out[s] = ok.mean() if len(ok) else float(d_lo)
    return out


def _determined(d_k, d_next):
    """The k-th and the (k+1)-th squared distance differ by more than their float32 rounding (three differences, three squares, two
    sums: 8 * 2^-24 relative on either)."""
    return d_next - d_k > 16 * U * d_next


def smooth(points, values, k):
    """(mean of ``values`` over the k nearest of ``points`` to each point (N,), neighbour set determined (N,) bool)."""
    d, idx, nxt = knn_brute(np.asarray(points)[None], np.asarray(points)[None], k)
    return np.asarray(values, np.float64)[idx[0]].mean(1), _determined(d[0][:, -1], nxt[0])


def vertex_values(verts, samples, values, k):
    """(assign_vertex_sdf in float64 (V,), neighbour set determined (V,) bool, the unscaled weighted means (V,))."""
    d, idx, nxt = knn_brute(np.asarray(verts)[None], np.asarray(samples)[None], k)
    w = 1.0 / (np.sqrt(d[0]) + 1e-6)
    w /= w.sum(1, keepdims=True)
    raw = (np.asarray(values, np.float64)[idx[0]] * w).sum(1)
    lo, hi = raw.min(), raw.max()
    return ((raw - lo) / (hi - lo) if hi > lo else np.zeros_like(raw)), _determined(d[0][:, -1], nxt[0]), raw


# ---- hand meshes on which float32 is exact -------------------------------------------------------------------------------------
def box(lo, hi):
    """(verts (8,3), faces (12,3)) of the axis-aligned box [lo, hi]^3 (or per-axis bounds), two triangles per side."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    v = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]])
    return v, f


def merge(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def evenly_spaced_faces(F, n=400):
    return np.unique(np.linspace(0, F - 1, min(n, F)).round().astype(np.int64))


def centroid_rays(verts, faces, face_idx, num_rays, seed):
    """Origins and inward-hemisphere unit directions (float32) for the centroids of ``face_idx``, as compute_sdf forms them, with
    directions from numpy's generator: (points, origins, dirs)."""
    v = np.asarray(verts, np.float32)
    fv = v[np.asarray(faces)[face_idx]]
    pts = fv.mean(1, dtype=np.float32)
    n = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    d = np.random.RandomState(seed).randn(len(face_idx), num_rays, 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=2, keepdims=True).astype(np.float32)
    d = np.where(((d * -n[:, None, :]).sum(-1) < 0)[..., None], -d, d).astype(np.float32)
    _, _, _, off = thresholds(v)
    return pts, (pts + n * off).astype(np.float32), d


# ---- the shared cases: computed once per process, never modified ----------------------------------------------------------------
def fixture_origins(g, name):
    """The ray origins of the fixture's run ``name`` ("all" / "sampled"), as compute_sdf forms them in float32."""
    v, f = g["verts"], g["faces"]
    fv = v[f[g[name + "_face_idx"]]]
    n = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    return (g[name + "_points"] + n * thresholds(v)[3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """The fixture's run ``name`` through ``cast`` with its recorded directions: (fixture, origins, cast result, float64 diameters)."""
    g = np.load(os.path.join(GOLDEN, "sdf_ray_ref.npz"))
    v, f = g["verts"], g["faces"]
    diag, d_lo, d_hi, off = thresholds(v)
    o = fixture_origins(g, name)
    c = cast(v, f, o, g[name + "_face_idx"], g[name + "_dirs"], off, d_lo, d_hi, diag)
    cap = max(len(o) // 2, 1)
    return g, o, c, diameters(c["t"], d_lo, d_hi, cap)


def load_mesh(name):
    """(verts float32, faces int64) of "fixture", "atta" (the scan under tests/golden) or "stick" (the model's template)."""
    if name == "fixture":
        g = np.load(os.path.join(GOLDEN, "sdf_ray_ref.npz"))
        return g["verts"], g["faces"]
    if name == "atta":
        g = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
        return g["verts"].astype(np.float32), g["faces"].astype(np.int64)
    z = np.load(MODEL_FILES[name], allow_pickle=True)
    return z["v_template"].astype(np.float32), z["faces"].astype(np.int64)


@functools.lru_cache(maxsize=None)
def condition_case(name, n_faces=400, num_rays=30, seed=0):
    """``n_faces`` evenly spaced faces of mesh ``name`` with ``num_rays`` rays each: dict of the mesh, the rays, the thresholds, the
    cast result and the float64 diameters (cap above num_rays)."""
    v, f = load_mesh(name)
    diag, d_lo, d_hi, off = thresholds(v)
    fi = evenly_spaced_faces(len(f), n_faces)
    pts, o, d = centroid_rays(v, f, fi, num_rays, seed)
    c = cast(v, f, o, fi, d, off, d_lo, d_hi, diag)
    cap = max(len(fi) // 2, 1)
    return dict(verts=v, faces=f, face_idx=fi, points=pts, origins=o, dirs=d, diag=diag, d_lo=d_lo, d_hi=d_hi, t_min=off, cap=cap, cast=c,
                diam=diameters(c["t"], d_lo, d_hi, cap))
