"""A restatement of the winding numbers of smilify_amd/csrc/point_mesh.hip (k_pm_winding) in numpy array operations, for tests: it
defines what the kernel computes, it is slow, and it runs anywhere.  It takes a dtype: float64 is the reference, float32 the
yardstick the kernel's error is measured with.  (With ``device`` the same operations run as torch tensor operations on that device,
so that a GPU test gets its float64 reference in no time; the CPU tests pin the numpy form.)

The rules (include/smilfit.h, smil_point_mesh_winding):

* The mesh and the cloud are brought into the mesh's FRAME first: every coordinate times 2^-ex, the power of two that brings the
  largest finite |coordinate| of the face vertices and the points below 1 (exact).
* Per pair, in ``dtype``, with a = v0 - p, b = a + e1, c = a + e2 (e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2):
  det = a . n, den = |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|, Omega / (4 pi) = atan2(det, den) / (2 pi)  (van Oosterom & Strackee).
* A pair with det == 0 (either sign of zero) adds exactly 0: a degenerate face, a point in the face's plane, a point on a vertex.
* A face with a non-finite vertex (or one above 3e38 in magnitude), or with a vertex index outside the mesh, adds 0.
* A point with such a coordinate gets NaN (and so does a padded one: the caller's business here).
* The sum is an INTEGER sum: every pair's value (|.| <= 0.5) times 2^fix, rounded to the nearest integer (ties to even), with
  fix = fix_unit_exp(0, F) = 61 - bits(F) of csrc/common.h; the total times 2^-fix, rounded once to ``dtype``.  A mesh without faces: 0.
"""
import numpy as np

U = 2.0 ** -24  # half an ulp of 1 in float32
USABLE = 3.0e38
INV_2PI = 0.15915494309189535


def fix_exp(n_faces: int) -> int:
    """fix_unit_exp(eb = 0, addends = max(F, 1)) of csrc/common.h: 61 - (64 - clzll(addends)) - eb."""
    return 61 - int(max(int(n_faces), 1)).bit_length() - 0


def frame_exp(verts, faces, points) -> int:
    """ex with every usable |coordinate| of the face vertices and the points < 2^ex (frexp of the largest; 0 for none)."""
    v, f, p = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(points, np.float64)
    ok = ((f >= 0) & (f < len(v))).all(-1)
    used = np.abs(np.concatenate([v[f[ok]].reshape(-1), p.reshape(-1)]))
    used = used[used <= USABLE]
    return int(np.frexp(np.float32(used.max()))[1]) if used.size and used.max() > 0 else int(np.frexp(np.float32(0.0))[1])


def _pair_values(xp, v0, e1, e2, nrm, p):
    """Omega / (4 pi) of every (point, face) pair: v0, e1, e2, nrm (1,F,3) and p (C,1,3) in one dtype -> (C,F)."""
    a = v0 - p
    b = a + e1
    c = a + e2
    dot = lambda x, y: x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]  # noqa: E731
    det = dot(a, nrm)
    la, lb, lc = xp.sqrt(dot(a, a)), xp.sqrt(dot(b, b)), xp.sqrt(dot(c, c))
    den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la
    ang = (xp.arctan2 if xp is np else xp.atan2)(det, den) * INV_2PI
    return xp.where(xp.abs(det) > 0, ang, xp.zeros_like(ang))  # (a NaN det - an unusable face or point - compares false: 0)


def winding(verts, faces, points, dtype=np.float64, device=None, chunk: int = 128):
    """The winding number (P,) of every point of one mesh: verts (V,3), faces (F,3), points (P,3), float32 data.  Returned as a numpy
    float64 array holding the values of ``dtype``.  ``device``: evaluate with torch on that device instead of numpy."""
    dtype = np.dtype(dtype)
    v32, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    if len(f) == 0 or len(p32) == 0:
        out = np.zeros(len(p32))
    else:
        scale = np.float64(2.0) ** -frame_exp(v32, f, p32)
        with np.errstate(invalid="ignore", over="ignore"):
            in_range = ((f >= 0) & (f < len(v32))).all(-1)
            tri = v32.astype(np.float64)[np.where(in_range[:, None], f, 0)]  # (F,3,3)
            tri[~(in_range & (np.abs(tri) <= USABLE).all(-1).all(-1))] = np.nan
            tri = (tri * scale).astype(dtype)  # the frame: exact
            pts = (p32.astype(np.float64) * scale).astype(dtype)
            v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                            e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        fix = fix_exp(len(f))
        if device is None:
            xp, tables = np, [t[None] for t in (v0, e1, e2, nrm)]
        else:
            import torch as xp

            tables = [xp.from_numpy(np.ascontiguousarray(t[None])).to(device) for t in (v0, e1, e2, nrm)]
            pts = xp.from_numpy(pts).to(device)
        acc = []
        for s in range(0, len(pts), chunk):
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                val = _pair_values(xp, *tables, pts[s:s + chunk, None, :])
                if xp is np:
                    acc.append(np.rint(val.astype(np.float64) * 2.0 ** fix).astype(np.int64).sum(1))
                else:
                    acc.append(xp.round(val.double() * 2.0 ** fix).long().sum(1).cpu().numpy())
        out = np.concatenate(acc).astype(np.float64) * 2.0 ** -fix
    out = out.astype(dtype).astype(np.float64)
    out[~(np.abs(p32) <= USABLE).all(-1)] = np.nan
    return out


def pair_value(tri, p, dtype=np.float64) -> float:
    """Omega / (4 pi) of ONE triangle (3,3) seen from ONE point, no frame and no integer sum (hand cases)."""
    t, q = np.asarray(tri, dtype), np.asarray(p, dtype)
    e1, e2 = t[1] - t[0], t[2] - t[0]
    return float(_pair_values(np, t[0][None, None], e1[None, None], e2[None, None], np.cross(e1, e2).astype(dtype)[None, None], q[None, None])[0, 0])
