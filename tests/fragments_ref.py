"""Test-side restatements for the fragment outputs (``engine.render_fragments``) and the depth visibility test
(``engine.depth_visibility``).  Test infrastructure only.

Fragments.  ``reference(name)`` adds, per image of a scene of tests/colour_cases.py, to the float64 restatement of the hard raster
(``shade_ref.raster_k1_detail``, cached by ``colour_cases.reference``): ``dist`` - the distance from the camera centre ``-T R^T`` to the
world point ``sum b_c X_c`` of every hit pixel - in float64, and ``zbuf32`` / ``bary32`` / ``dist32``: the same formulas evaluated in numpy
float32 from the float32 inputs for the restatement's winner (its face and, for a cut face, its part).  The float32 evaluation is the
yardstick of the GPU test, as ``shade_ref.shade(dtype=np.float32)`` is for colour: it shows what float32 itself costs on the scene.

Visibility.  ``visibility_rules`` restates smal_fitter/Unreal2Pytorch3D.py:733-758 for one image from the keypoints' distances,
``refine_visibility`` from their 3-D points and the camera location as the reference takes them, ``*_batch`` over a leading image axis.
``dtype=np.float32`` evaluates the distance, the decoded surface and the comparison in float32: what the test must NOT be run in.
"""
import functools
from types import SimpleNamespace

import numpy as np

import colour_cases as cc
import shade_ref

FRAGMENT_SCENES = ["partial9", "partial17", "partial65", "overflow", "ties_batches", "stack129_partial", "cuts", "degenerate",
                   "cameras_N", "cameras_1", "cameras_views"]
FLOOR = 2.0 ** -21   # the floor of the colour edge tests: relative to the scene's largest depth for zbuf / dist, absolute for bary


# ----------------------------------------------------------------------------------------------
# fragments
# ----------------------------------------------------------------------------------------------
def clip_face(ndc, tri, z_clip, dtype):
    """clip_faces for ONE face in ``dtype``: a list over its front parts of ``(tri (3,3), conv (3,3))`` as ``shade_ref.clip_mesh``
    forms them (row s of ``conv``: part vertex s in barycentrics of the face), every step rounded to ``dtype``."""
    f = dtype
    P = ndc[tri].astype(f)
    z = P[:, 2]
    eye = np.eye(3, dtype=f)
    behind = z < f(z_clip)
    nb = int(behind.sum())
    if nb == 0:
        return [(P, eye)]
    if nb == 3:
        return []
    k = int(np.nonzero(behind)[0][0]) if nb == 1 else int(np.nonzero(~behind)[0][0])
    c1, c2, c3 = k, (k + 1) % 3, (k + 2) % 3
    zc = f(z_clip)

    def cross(a, b):
        t = (z[a] - zc) / (z[a] - z[b])
        ca, cb = z[a] * (f(1.0) - t) / zc, z[b] * t / zc
        p = np.array([ca * P[a, 0] + cb * P[b, 0], ca * P[a, 1] + cb * P[b, 1], zc], f)
        return p, (f(1.0) - t) * eye[a] + t * eye[b]

    q4, q5 = cross(c1, c2), cross(c1, c3)
    V = {c: (P[c], eye[c]) for c in range(3)}
    parts = [[q4, V[c2], V[c3]], [q4, V[c3], q5]] if nb == 1 else [[V[c1], q4, q5]]
    return [(np.stack([q[0] for q in part]).astype(f), np.stack([q[1] for q in part]).astype(f)) for part in parts]


def winner_terms(p2f, part, ndc, faces, S, dtype, z_clip=shade_ref.Z_CLIP):
    """``(zbuf (S,S), bary (S,S,3))`` in ``dtype`` of the given winners (face ``p2f``, part ``part`` as ``raster_k1_detail`` names it): the
    rasteriser's formulas - edge functions over area + eps, perspective correction, depth, map-back through ``conv`` - evaluated in
    ``dtype`` from ``ndc`` rounded to ``dtype``.  Pixels without a hit hold NaN."""
    f = dtype
    g = shade_ref._pix_ndc(S).astype(f)
    eps = f(shade_ref.EPS)
    zbuf, bary = np.full((S, S), np.nan, f), np.full((S, S, 3), np.nan, f)
    ndc = np.asarray(ndc).astype(f)
    for face in np.unique(p2f[p2f >= 0]):
        parts = clip_face(ndc, np.asarray(faces)[face], z_clip, f)
        for pj in np.unique(part[p2f == face]):
            tri, conv = parts[max(int(pj), 0)]
            yo, xo = np.nonzero((p2f == face) & (part == pj))
            px, py = g[xo], g[yo]
            x, y, z = tri[:, 0], tri[:, 1], tri[:, 2]
            ar = ((x[2] - x[0]) * (y[1] - y[0]) - (y[2] - y[0]) * (x[1] - x[0])) + eps
            e = lambda ax, ay, bx, by: (px - ax) * (by - ay) - (py - ay) * (bx - ax)  # noqa: E731
            b0, b1, b2 = e(x[1], y[1], x[2], y[2]) / ar, e(x[2], y[2], x[0], y[0]) / ar, e(x[0], y[0], x[1], y[1]) / ar
            w0, w1, w2 = b0 * z[1] * z[2], b1 * z[0] * z[2], b2 * z[0] * z[1]
            den = np.maximum(w0 + w1 + w2, eps)
            p = np.stack([w0 / den, w1 / den, w2 / den], -1)
            zbuf[yo, xo] = p[:, 0] * z[0] + p[:, 1] * z[1] + p[:, 2] * z[2]
            bary[yo, xo] = p[:, 0:1] * conv[0] + p[:, 1:2] * conv[1] + p[:, 2:3] * conv[2]   # (elementwise: no BLAS, the same bits everywhere)
    assert zbuf.dtype == f and bary.dtype == f
    return zbuf, bary


def distance(p2f, bary, verts_world, faces, R, T, dtype):
    """(S,S) distance from the camera centre ``-T R^T`` to ``sum_c bary_c verts_world[face_c]`` in ``dtype`` (+inf: no hit)."""
    f = dtype
    hit = p2f >= 0
    out = np.full(p2f.shape, np.inf, f)
    vw = np.asarray(verts_world).astype(f)
    b, tri = bary[hit].astype(f), vw[np.asarray(faces)[p2f[hit]]]
    pts = b[:, 0:1] * tri[:, 0] + b[:, 1:2] * tri[:, 1] + b[:, 2:3] * tri[:, 2]   # (elementwise sums: no BLAS, the same bits everywhere)
    R, T = np.asarray(R).astype(f), np.asarray(T).astype(f)
    C = -(T[0] * R[:, 0] + T[1] * R[:, 1] + T[2] * R[:, 2])
    out[hit] = np.sqrt(((C[None] - pts) ** 2).sum(-1))
    assert out.dtype == f
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per image of the scene: the namespace of ``colour_cases.reference`` (not modified) extended by ``dist`` (float64), ``zbuf32``,
    ``bary32`` and ``dist32`` (the float32 yardstick at the restatement's winner)."""
    s = cc.get(name)
    out = []
    for n, r in enumerate(cc.reference(name)):
        vw, R, T = s.verts_world[n // s.views], s.R[n % len(s.R)], s.T[n % len(s.T)]
        z32, b32 = winner_terms(r.pix_to_face, r.part, s.verts_ndc[n], s.faces, s.S, np.float32)
        out.append(SimpleNamespace(**vars(r), dist=distance(r.pix_to_face, r.bary, vw, s.faces, R, T, np.float64), zbuf32=z32, bary32=b32,
                                   dist32=distance(r.pix_to_face, b32, vw, s.faces, R, T, np.float32)))
    return out


def yardstick(name):
    """``(err_zbuf, err_bary, err_dist, largest zbuf, largest dist)`` of the float32 evaluation against float64 over the scene's hit
    pixels that are not ``unsure``."""
    ez = eb = ed = zmax = dmax = 0.0
    for r in reference(name):
        ok = (r.pix_to_face >= 0) & ~r.unsure
        if ok.any():
            ez = max(ez, float(np.abs(r.zbuf32[ok] - r.zbuf[ok]).max()))
            eb = max(eb, float(np.abs(r.bary32[ok] - r.bary[ok]).max()))
            ed = max(ed, float(np.abs(r.dist32[ok] - r.dist[ok]).max()))
            zmax, dmax = max(zmax, float(r.zbuf[ok].max())), max(dmax, float(r.dist[ok].max()))
    return ez, eb, ed, zmax, dmax


# ----------------------------------------------------------------------------------------------
# depth visibility
# ----------------------------------------------------------------------------------------------
def visibility_rules(visibility, kp_norm, kp_dist, depth, neighborhood, tolerance, depth_max=None, dtype=np.float64):
    """One image.  ``depth`` (H,W,C) uint8 with ``depth_max`` (the depth in channel 0) or (H,W) float distances; ``kp_norm`` (P,2) =
    (row / H, column / W); ``kp_dist`` (P,).  Returns ``(visibility out (P,) float32, surface (P,) dtype: NaN where not sampled)``."""
    f = dtype
    vis = np.array(visibility, np.float32)
    surface = np.full(len(vis), np.nan, f)
    H, W = depth.shape[:2]
    u8 = depth.dtype == np.uint8
    h = max(int(neighborhood), 0)
    for j in range(len(vis)):
        d = f(kp_dist[j])
        nx, ny = float(kp_norm[j][0]), float(kp_norm[j][1])
        if vis[j] == 0.0 or not np.isfinite(d) or not (0.0 <= nx <= 1.0 and 0.0 <= ny <= 1.0):
            continue
        row, col = min(max(int(nx * H), 0), H - 1), min(max(int(ny * W), 0), W - 1)
        win = depth[max(0, row - h):min(H, row + h + 1), max(0, col - h):min(W, col + h + 1)]
        if u8:
            surface[j] = (f(int(win[..., 0].min())) / f(255.0)) * f(depth_max)
        else:
            surface[j] = f(win.min())
        if d > surface[j] + f(tolerance):
            vis[j] = 0.0
    return vis, surface


def point_distances(points, camera, dtype=np.float64):
    """(...,P) distances of ``points`` (...,P,3) to ``camera`` (...,3) in ``dtype`` (NaN for a non-finite point)."""
    diff = np.asarray(points).astype(dtype) - np.asarray(camera).astype(dtype)[..., None, :]
    with np.errstate(invalid="ignore"):
        d = np.sqrt((diff * diff).sum(-1))
    return np.where(np.isfinite(np.asarray(points)).all(-1), d, dtype(np.nan)).astype(dtype)


def refine_visibility(visibility, kp_norm, points, camera, depth, neighborhood, tolerance, depth_max=None, dtype=np.float64):
    """``visibility_rules`` from the 3-D points and the camera location, as the reference function takes them."""
    return visibility_rules(visibility, kp_norm, point_distances(points, camera, dtype), depth, neighborhood, tolerance, depth_max, dtype)


def visibility_rules_batch(visibility, kp_norm, kp_dist, depth, neighborhood, tolerance, depth_max=None, dtype=np.float64):
    """Leading image axis on every array: ``(visibility out (B,P), surface (B,P))``."""
    res = [visibility_rules(visibility[b], kp_norm[b], kp_dist[b], depth[b], neighborhood, tolerance, depth_max, dtype) for b in range(len(depth))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def refine_visibility_batch(visibility, kp_norm, points, camera, depth, neighborhood, tolerance, depth_max=None, dtype=np.float64):
    return visibility_rules_batch(visibility, kp_norm, point_distances(points, camera, dtype), depth, neighborhood, tolerance, depth_max, dtype)


def encode_depth_u8(dist, depth_max):
    """numpy form of ``smilify_amd.visibility.encode_depth_u8``: round to nearest, +inf -> 255."""
    with np.errstate(invalid="ignore"):
        q = np.floor(np.asarray(dist, np.float64) / float(depth_max) * 255.0 + 0.5)
    return np.clip(np.where(np.isfinite(q), q, 255.0), 0.0, 255.0).astype(np.uint8)


# ----------------------------------------------------------------------------------------------
# the model scene of Renderer.keypoint_visibility
# ----------------------------------------------------------------------------------------------
VIS_S, VIS_FRAMES, VIS_VIEWS, VIS_TOLERANCE, VIS_NEIGHBORHOOD = 33, 2, 3, 0.05, 1
VIS_MARGIN_REL, VIS_MARGIN_PX = 1e-3, 0.05


@functools.lru_cache(maxsize=None)
def visibility_scene():
    """The sphere of colour_cases (radius 0.6, one per frame) seen by three cameras on ``synthetic.camera_ring`` at S = 33, and per frame
    eight points placed with respect to camera 0: in front of the sphere, behind it, on its far surface, beside its silhouette, outside
    the image, in front with visibility 0 coming in, just above the near surface and 0.1 under it (deeper than the tolerance 0.05).
    The other two cameras see the same points from 120 degrees to either side.  ``expected`` (N,P) and ``surface`` (N,P) come from the
    float64 restatement: the raster of the float32 NDC vertices, its distance map, ``visibility_rules`` on it."""
    import torch

    from oracle import render_ref
    from smilify_amd import synthetic

    S, frames, views = VIS_S, VIS_FRAMES, VIS_VIEWS
    N = frames * views
    R, T = synthetic.camera_ring(views, 2.7)
    R, T = R.numpy().astype(np.float32), T.numpy().astype(np.float32)
    fov = np.array([60.0], np.float32)
    centres = np.array([[0.05 + cc.O1, -0.04 + cc.O2, 0.03], [-0.07 + cc.O2, 0.06 + cc.O3, -0.05]])
    spheres = [cc._sphere(0.6, c, seed=31 + k) for k, c in enumerate(centres)]
    verts, faces = np.stack([v for v, _ in spheres]).astype(np.float32), spheres[0][1].astype(np.int32)
    cam0 = -T[0].astype(np.float64) @ R[0].astype(np.float64).T
    points = []
    for c in centres:
        d = (cam0 - c) / np.linalg.norm(cam0 - c)                 # towards camera 0
        side = np.cross(d, [0.0, 1.0, 0.0])
        side /= np.linalg.norm(side)
        up = np.cross(side, d)
        points.append([c + 0.9 * d + 0.02 * up, c - 0.9 * d + 0.03 * side, c - 0.585 * d + 0.02 * side, c + 0.78 * side + 0.1 * up,
                       c + 2.6 * side, c + 0.85 * d - 0.03 * up, c + 0.66 * d + 0.04 * side, c + 0.47 * d - 0.02 * up])
    img = np.arange(N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

    def screen(pts):  # (frames,P,3) float32 -> (N,P,2) (y, x) pixels in float64
        return render_ref.project_points_screen(t(pts).double().repeat_interleave(views, 0), t(R[img % views]).double(), t(T[img % views]).double(),
                                                t(fov).double(), S).numpy()

    # every point is moved by a seeded offset of about 0.01 until all of its projections keep VIS_MARGIN_PX from a pixel boundary
    rng = np.random.default_rng(5)
    points = np.asarray(points, np.float32)
    for k in range(frames):
        for j in range(points.shape[1]):
            for _ in range(200):
                cand = (points[k, j] + rng.normal(0.0, 0.01, 3)).astype(np.float32)
                yx = screen(np.broadcast_to(cand, (frames, 1, 3)))[k * views:(k + 1) * views]
                frac = yx - np.floor(yx)
                if np.minimum(frac, 1.0 - frac).min() >= 2.0 * VIS_MARGIN_PX:
                    points[k, j] = cand
                    break
            else:
                raise AssertionError((k, j))
    vis_in = np.ones((N, points.shape[1]), np.float32)
    vis_in[:, 5] = 0.0
    ndc = render_ref.project_to_ndc(t(verts).repeat_interleave(views, 0), t(R[img % views]), t(T[img % views]), t(fov)).numpy()
    yx = screen(points)
    kp_norm = yx / float(S)
    cams = -np.einsum("nk,nqk->nq", T[img % views].astype(np.float64), R[img % views].astype(np.float64))
    kp_dist = np.linalg.norm(points.astype(np.float64)[img // views] - cams[:, None], axis=-1)
    detail = [shade_ref.raster_k1_detail(ndc[n].astype(np.float64), faces, S) for n in range(N)]
    dist_map = np.stack([distance(d["pix_to_face"], d["bary"], verts[n // views], faces, R[n % views], T[n % views], np.float64)
                         for n, d in enumerate(detail)])
    expected, surface = visibility_rules_batch(vis_in, kp_norm, kp_dist, dist_map, VIS_NEIGHBORHOOD, VIS_TOLERANCE)
    return SimpleNamespace(S=S, frames=frames, views=views, N=N, R=R, T=T, fov=fov, verts=verts, faces=faces, points=points, vis_in=vis_in,
                           verts_ndc=ndc, yx=yx, kp_norm=kp_norm, kp_dist=kp_dist, unsure=np.stack([d["unsure"] for d in detail]),
                           dist_map=dist_map, expected=expected, surface=surface)


def visibility_scene_margins(s):
    """``(smallest relative distance of a sampled keypoint from its threshold, smallest distance in pixels of a projection from a pixel
    boundary or from the image's border, number of ``unsure`` pixels inside the keypoints' windows)``."""
    S, h = s.S, VIS_NEIGHBORHOOD
    sampled = np.isfinite(s.surface)
    thr = s.surface[sampled] + VIS_TOLERANCE
    rel = float((np.abs(s.kp_dist[sampled] - thr) / thr).min())
    frac = s.yx - np.floor(s.yx)
    px = float(min(np.minimum(frac, 1.0 - frac).min(), np.abs(s.yx).min(), np.abs(s.yx - S).min()))
    unsure = 0
    for n in range(s.N):
        for y, x in s.yx[n]:
            if 0.0 <= y <= S and 0.0 <= x <= S:
                r, c = min(int(y), S - 1), min(int(x), S - 1)
                unsure += int(s.unsure[n, max(0, r - h):r + h + 1, max(0, c - h):c + h + 1].sum())
    return rel, px, unsure
