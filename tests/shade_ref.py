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


_EYE = np.eye(3)                 # the barycentric map of a face that is not cut (clip_mesh hands out this very object)


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), x.dtype.type(N_EPS))


def vertex_normals(verts, faces, dtype=np.float64):
    """Meshes.verts_normals_packed: every corner adds its face's cross(v2 - v1, v0 - v1), then F.normalize(eps=1e-6)."""
    v = np.asarray(verts).astype(dtype)[np.asarray(faces)]
    n = np.cross(v[:, 2] - v[:, 1], v[:, 0] - v[:, 1])
    out = np.zeros((len(verts), 3), dtype)
    for k in range(3):
        np.add.at(out, np.asarray(faces)[:, k], n)
    return _normalize(out)


def clip_mesh(ndc, faces, z_clip=Z_CLIP):
    """clip_faces for one image in (x_ndc, y_ndc, z_view): a list of ``(tri (3,3) ndc, parent face, part, conv (3,3))`` in pytorch3d's
    order, row s of ``conv`` the barycentric coordinates of part vertex s with respect to the parent face."""
    ndc = np.asarray(ndc, np.float64)
    out = []
    eye = _EYE
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


def raster_k1_detail(ndc, faces, S, z_clip=Z_CLIP, dup_of=None):
    """Hard K = 1 raster of one image, with what the edge tests need to know about every pixel.  A dict of (S,S) arrays (``bary``
    (S,S,3)):

    ``pix_to_face``  original face id (-1: none); ``bary`` with respect to the original face; ``zbuf``.
    ``part``         -1 where the winner is a whole face, else its index (0, 1) among the front parts of its cut parent.
    ``second``       parent of the second-nearest candidate (-1: none).
    ``unsure``       pixels where the answer hangs on rounding: a depth near-tie with another candidate, or a barycentric within
                     ``EDGE_TOL`` of 0 for a face whose box holds the pixel.
    ``unsure_face``  the subset where the FACE hangs on rounding.  It leaves out what only decides between the two front parts of
                     one cut face (their shared diagonal, or a near-tie of the two): either part reports the same original face.
    ``tie``          with ``dup_of`` (F,), which maps every face to the lowest id among its declared bit-identical copies (same
                     vertex ids in the same order, hence the same depth to the bit in any arithmetic): hit pixels where a copy of
                     the winner has exactly the winner's depth.  Such a tie is no near-tie - the rule (smallest depth, then lowest
                     face) decides it - so it does not make a pixel ``unsure``; the winner is the lowest id."""
    g = _pix_ndc(S)
    p2f = np.full((S, S), -1, np.int64)
    part_of = np.full((S, S), -1, np.int64)
    second = np.full((S, S), -1, np.int64)
    bary = np.zeros((S, S, 3))
    zbuf = np.full((S, S), np.inf)
    z2 = np.full((S, S), np.inf)      # second-smallest candidate depth
    near_any = np.zeros((S, S), bool)
    near_ext = np.zeros((S, S), bool)
    tie = np.zeros((S, S), bool)
    if dup_of is not None:
        dup_of = np.asarray(dup_of, np.int64)
    clipped = clip_mesh(ndc, faces, z_clip)
    two_parts = {parent for _, parent, part, _ in clipped if part == 1}
    for tri, parent, part, conv in clipped:
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
        near = np.abs(p) < EDGE_TOL
        near_edge = near.any(-1) & (p > -EDGE_TOL).all(-1)
        Y, X = np.meshgrid(yo, xo, indexing="ij")
        near_any[Y[near_edge], X[near_edge]] = True
        if parent in two_parts:  # the diagonal of the quadrilateral: opposite corner 1 of part 0, corner 2 of part 1
            outer = near.copy()
            outer[..., 1 + part] = False
            near_edge = near_edge & outer.any(-1)
        near_ext[Y[near_edge], X[near_edge]] = True
        zb, zs, wp, ps = zbuf[Y, X], z2[Y, X], p2f[Y, X], second[Y, X]
        win = inside & (pz < zb)
        copy = np.zeros_like(win)
        if dup_of is not None:
            copy = inside & (pz == zb) & (wp >= 0) & (dup_of[np.maximum(wp, 0)] == dup_of[parent])
        behind = inside & ~win & ~copy & (pz < zs)
        z2[Y, X] = np.where(win, zb, np.where(behind, pz, zs))
        second[Y, X] = np.where(win, wp, np.where(behind, parent, ps))
        tie[Y[win], X[win]] = False
        tie[Y[copy], X[copy]] = True
        zbuf[Y[win], X[win]] = pz[win]
        p2f[Y[win], X[win]] = parent
        part_of[Y[win], X[win]] = -1 if conv is _EYE else part
        bary[Y[win], X[win]] = p[win] @ conv
    hit = p2f >= 0
    with np.errstate(invalid="ignore"):  # (inf - inf where a pixel has no second candidate)
        near_tie = hit & np.isfinite(z2) & (z2 - zbuf < TIE_REL * np.abs(zbuf))
    return dict(pix_to_face=p2f, bary=bary, zbuf=zbuf, part=part_of, second=second, tie=tie, unsure=near_any | near_tie,
                unsure_face=near_ext | (near_tie & (second != p2f)))


def raster_k1(ndc, faces, S, z_clip=Z_CLIP):
    """Hard K = 1 raster of one image.  Returns ``pix_to_face (S,S)`` original ids (-1: none), ``bary (S,S,3)`` with respect to the
    original face, ``zbuf (S,S)`` and ``unsure (S,S)``: pixels where the answer hangs on rounding - a depth near-tie with another
    candidate, or a barycentric within ``EDGE_TOL`` of 0 for a face whose box holds the pixel."""
    r = raster_k1_detail(ndc, faces, S, z_clip)
    return r["pix_to_face"], r["bary"], r["zbuf"], r["unsure"]


def shade_terms(p2f, bary, verts_world, faces, R, T, dtype=np.float64):
    """The HardPhong terms of every hit pixel, in ``dtype`` from inputs rounded to ``dtype``: a dict of (h,) arrays in the order of
    ``np.nonzero(p2f >= 0)`` - ``bsum`` = b0 + b1 + b2, ``nlen`` the length of the interpolated normal before it is normalised,
    ``cos`` = n.d, ``vr`` = v.r (not gated), ``spec`` the gated specular term 0.2 (relu(v.r) [n.d > 0])^64."""
    f = dtype
    hit = p2f >= 0
    vw = np.asarray(verts_world).astype(f)
    fc = np.asarray(faces)[p2f[hit]]                       # (h,3)
    b = bary[hit].astype(f)                                # (h,3)
    normals = vertex_normals(vw, faces, dtype=f)
    pts = np.einsum("hk,hkc->hc", b, vw[fc])
    raw = np.einsum("hk,hkc->hc", b, normals[fc])
    nrm = _normalize(raw)
    R, T = np.asarray(R).astype(f), np.asarray(T).astype(f)
    C = -T @ R.T
    d = _normalize(LIGHT.astype(f)[None] - pts)
    v = _normalize(C[None] - pts)
    cos = (nrm * d).sum(-1)
    r = -d + f(2.0) * cos[:, None] * nrm
    vr = (v * r).sum(-1)
    alpha = np.maximum(vr, f(0.0)) * (cos > 0)
    return dict(bsum=b.sum(-1), nlen=np.linalg.norm(raw, axis=-1), cos=cos, vr=vr, spec=f(SPECULAR) * alpha ** SHININESS)


def shade(p2f, bary, verts_world, faces, R, T, rgb, dtype=np.float64):
    """HardPhong of the raster result: (3,S,S), background 1.  ``dtype=np.float32`` evaluates the same formulas in float32 from
    float32 inputs (at the given barycentrics): what float32 itself costs, the yardstick of the shading tests."""
    S = p2f.shape[0]
    img = np.ones((S, S, 3), dtype)
    hit = p2f >= 0
    if not hit.any():
        return img.transpose(2, 0, 1)
    t = shade_terms(p2f, bary, verts_world, faces, R, T, dtype)
    diffuse = dtype(DIFFUSE) * np.maximum(t["cos"], dtype(0.0))
    texel = np.asarray(rgb).astype(dtype)[None] * t["bsum"][:, None]
    img[hit] = (dtype(AMBIENT) + diffuse)[:, None] * texel + t["spec"][:, None]
    return img.transpose(2, 0, 1)


def render_colour(verts_world, ndc, faces, R, T, rgb, S, z_clip=Z_CLIP):
    """One image: ``verts_world (V,3)`` of its frame, ``ndc (V,3)`` = (x_ndc, y_ndc, z_view) through its camera ``R (3,3)``, ``T (3,)``.
    Returns ``(image (3,S,S), pix_to_face (S,S), unsure (S,S))``."""
    p2f, bary, _, unsure = raster_k1(ndc, faces, S, z_clip)
    return shade(p2f, bary, verts_world, faces, R, T, rgb), p2f, unsure
