"""Float64 numpy restatement of the reference Renderer's colour branch (smal_fitter/p3d_renderer.py:54-70,148-150), for tests only.

pytorch3d 0.7.x (not installed here; PARITY UNPINNED, as for the silhouette oracle) restated from its published algorithm:

* ``MeshRasterizer`` with ``blur_radius=0, faces_per_pixel=1, bin_size=0``: perspective-correct barycentrics, not clipped, ``z_clip =
  znear / 2``, no culling.  A pixel keeps a face only when it is strictly inside (all three corrected barycentrics > 0) and ``pz >= 0``;
  the naive kernel visits the faces in order and replaces on a strictly smaller depth, so the smallest ``(z, face)`` wins.
* ``clip_faces``: faces with all vertices nearer than ``z_clip`` are dropped, a face that crosses it is replaced by its front part (one
  triangle, or a quadrilateral as two) at its own place in the face order; ``convert_clipped_rasterization_to_original_faces`` maps the
  part's barycentrics back to the face (each part vertex is a known barycentric point of it).
* ``HardPhongShader(lights=PointLights(location=[[0, 0, 3]]))`` with default ``Materials`` / ``BlendParams`` over ``TexturesVertex`` of
  one colour: ``colour = (0.5 + 0.3 relu(n.d)) rgb (b0 + b1 + b2) + 0.2 (relu(v.r) [n.d > 0])^64``, background (1, 1, 1); normals are
  ``Meshes.verts_normals_packed`` interpolated with the barycentrics, points likewise, in world space; camera centre ``-T R^T``.

Pixel centres and orientation as on the silhouette path: output column ``xo`` is image x index ``S - 1 - xo`` with NDC
``-1 + (2 i + 1) / S`` (rows likewise).
"""
from __future__ import annotations

import numpy as np

Z_CLIP = 5e-4                    # znear / 2 (reference znear = 1e-3)
LIGHT = np.array([0.0, 0.0, 3.0])
AMBIENT, DIFFUSE, SPECULAR, SHININESS = 0.5, 0.3, 0.2, 64
EPS = 1e-8                       # rasteriser kEpsilon
N_EPS = 1e-6                     # F.normalize eps
TIE_REL = 1e-6                   # a depth near-tie: |dz| < TIE_REL * z
EDGE_TOL = 1e-6                  # a barycentric within this of 0


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), N_EPS)


def vertex_normals(verts, faces):
    """Meshes.verts_normals_packed: every corner adds its face's cross(v2 - v1, v0 - v1), then F.normalize(eps=1e-6)."""
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    n = np.cross(v[:, 2] - v[:, 1], v[:, 0] - v[:, 1])
    out = np.zeros((len(verts), 3))
    for k in range(3):
        np.add.at(out, np.asarray(faces)[:, k], n)
    return _normalize(out)


def clip_mesh(ndc, faces, z_clip=Z_CLIP):
    """clip_faces for one image in (x_ndc, y_ndc, z_view): a list of ``(tri (3,3) ndc, parent face, part, conv (3,3))`` in pytorch3d's
    order, row s of ``conv`` the barycentric coordinates of part vertex s with respect to the parent face."""
    ndc = np.asarray(ndc, np.float64)
    out = []
    eye = np.eye(3)
    for f, tri in enumerate(np.asarray(faces)):
        z = ndc[tri, 2]
        behind = z < z_clip
        nb = int(behind.sum())
        if nb == 0:
            out.append((ndc[tri], f, 0, eye))
            continue
        if nb == 3:
            continue
        k = int(np.nonzero(behind)[0][0]) if nb == 1 else int(np.nonzero(~behind)[0][0])  # the isolated corner
        c1, c2, c3 = k, (k + 1) % 3, (k + 2) % 3

        def cross(a, b):  # where edge (corner a, corner b) meets the plane; view-space interpolation
            za, zb = z[a], z[b]
            t = (za - z_clip) / (za - zb)
            ca, cb = za * (1.0 - t) / z_clip, zb * t / z_clip
            p = np.array([ca * ndc[tri[a], 0] + cb * ndc[tri[b], 0], ca * ndc[tri[a], 1] + cb * ndc[tri[b], 1], z_clip])
            return p, (1.0 - t) * eye[a] + t * eye[b]

        p4, b4 = cross(c1, c2)
        p5, b5 = cross(c1, c3)
        P = {c: (ndc[tri[c]], eye[c]) for c in range(3)}
        if nb == 1:
            parts = [[(p4, b4), P[c2], P[c3]], [(p4, b4), P[c3], (p5, b5)]]
        else:
            parts = [[P[c1], (p4, b4), (p5, b5)]]
        for j, part in enumerate(parts):
            out.append((np.stack([q[0] for q in part]), f, j, np.stack([q[1] for q in part])))
    return out


def _pix_ndc(S):
    return -1.0 + (2.0 * (S - 1 - np.arange(S)) + 1.0) / S   # output index -> NDC (mirrored)


def raster_k1(ndc, faces, S, z_clip=Z_CLIP):
    """Hard K = 1 raster of one image.  Returns ``pix_to_face (S,S)`` original ids (-1: none), ``bary (S,S,3)`` with respect to the
    original face, ``zbuf (S,S)`` and ``unsure (S,S)``: pixels where the answer hangs on rounding - a depth near-tie with another
    candidate, or a barycentric within ``EDGE_TOL`` of 0 for a face whose box holds the pixel."""
    g = _pix_ndc(S)
    p2f = np.full((S, S), -1, np.int64)
    bary = np.zeros((S, S, 3))
    zbuf = np.full((S, S), np.inf)
    z2 = np.full((S, S), np.inf)      # second-smallest candidate depth
    unsure = np.zeros((S, S), bool)
    for tri, parent, part, conv in clip_mesh(ndc, faces, z_clip):
        x, y, z = tri[:, 0], tri[:, 1], tri[:, 2]
        if z.min() < EPS or z.max() < z_clip:
            continue
        area = (x[2] - x[0]) * (y[1] - y[0]) - (y[2] - y[0]) * (x[1] - x[0])
        if abs(area) <= EPS:
            continue
        # pixel window: box of the triangle plus one pixel (output indices)
        lo = lambda v: int(np.floor(((v + 1.0) * S - 1.0) / 2.0)) - 1  # noqa: E731
        xi0, xi1 = max(lo(x.min()), 0), min(lo(x.max()) + 3, S - 1)
        yi0, yi1 = max(lo(y.min()), 0), min(lo(y.max()) + 3, S - 1)
        if xi0 > xi1 or yi0 > yi1:
            continue
        xo = np.arange(S - 1 - xi1, S - xi0)
        yo = np.arange(S - 1 - yi1, S - yi0)
        px, py = g[xo][None, :], g[yo][:, None]
        ar = area + EPS
        e = lambda ax, ay, bx, by: (px - ax) * (by - ay) - (py - ay) * (bx - ax)  # noqa: E731
        b0 = e(x[1], y[1], x[2], y[2]) / ar
        b1 = e(x[2], y[2], x[0], y[0]) / ar
        b2 = e(x[0], y[0], x[1], y[1]) / ar
        w0, w1, w2 = b0 * z[1] * z[2], b1 * z[0] * z[2], b2 * z[0] * z[1]
        den = np.maximum(w0 + w1 + w2, EPS)
        p = np.stack([w0 / den, w1 / den, w2 / den], -1)
        pz = p[..., 0] * z[0] + p[..., 1] * z[1] + p[..., 2] * z[2]
        inside = (p > 0).all(-1) & (pz >= 0)
        near_edge = (np.abs(p) < EDGE_TOL).any(-1) & (p > -EDGE_TOL).all(-1)
        Y, X = np.meshgrid(yo, xo, indexing="ij")
        unsure[Y[near_edge], X[near_edge]] = True
        zb, zs = zbuf[Y, X], z2[Y, X]
        win = inside & (pz < zb)
        new_z2 = np.where(win, zb, np.where(inside, np.minimum(zs, pz), zs))
        z2[Y, X] = new_z2
        zbuf[Y[win], X[win]] = pz[win]
        p2f[Y[win], X[win]] = parent
        bary[Y[win], X[win]] = p[win] @ conv
    hit = p2f >= 0
    with np.errstate(invalid="ignore"):  # (inf - inf where a pixel has no second candidate)
        unsure |= hit & np.isfinite(z2) & (z2 - zbuf < TIE_REL * np.abs(zbuf))
    return p2f, bary, zbuf, unsure


def shade(p2f, bary, verts_world, faces, R, T, rgb):
    """HardPhong of the raster result: (3,S,S), background 1."""
    S = p2f.shape[0]
    img = np.ones((S, S, 3))
    hit = p2f >= 0
    if not hit.any():
        return img.transpose(2, 0, 1)
    vw = np.asarray(verts_world, np.float64)
    fc = np.asarray(faces)[p2f[hit]]                      # (h,3)
    b = bary[hit]                                          # (h,3)
    normals = vertex_normals(vw, faces)
    pts = np.einsum("hk,hkc->hc", b, vw[fc])
    nrm = _normalize(np.einsum("hk,hkc->hc", b, normals[fc]))
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64)
    C = -T @ R.T
    d = _normalize(LIGHT[None] - pts)
    v = _normalize(C[None] - pts)
    cos = (nrm * d).sum(-1)
    diffuse = DIFFUSE * np.maximum(cos, 0.0)
    r = -d + 2.0 * cos[:, None] * nrm
    alpha = np.maximum((v * r).sum(-1), 0.0) * (cos > 0)
    spec = SPECULAR * alpha ** SHININESS
    texel = np.asarray(rgb, np.float64)[None] * b.sum(-1, keepdims=True)
    img[hit] = (AMBIENT + diffuse)[:, None] * texel + spec[:, None]
    return img.transpose(2, 0, 1)


def render_colour(verts_world, ndc, faces, R, T, rgb, S, z_clip=Z_CLIP):
    """One image: ``verts_world (V,3)`` of its frame, ``ndc (V,3)`` = (x_ndc, y_ndc, z_view) through its camera ``R (3,3)``, ``T (3,)``.
    Returns ``(image (3,S,S), pix_to_face (S,S), unsure (S,S))``."""
    p2f, bary, _, unsure = raster_k1(ndc, faces, S, z_clip)
    return shade(p2f, bary, verts_world, faces, R, T, rgb), p2f, unsure
