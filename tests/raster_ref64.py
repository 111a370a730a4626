"""TEST INFRASTRUCTURE ONLY: a float64 restatement of the soft-silhouette rasteriser with an autograd gradient.

Independent of the product and of ``oracle/raster_oracle.c`` (it imports neither): dense torch float64 on the CPU, one image at a
time, every (pixel, face) pair evaluated, chunked over pixel rows so that the peak stays under about 1 GB.  It restates the published
algorithm that DESIGN 4.2 and the header of ``oracle/raster_oracle.c`` state:

* pixel centre ``-1 + (2 i + 1) / S`` on flipped axes (output row 0 is the top row, NDC +x is left);
* a face is skipped if ``zmin < 1e-8``, ``zmax < z_clip`` or ``|area| <= 1e-8``; barycentrics over ``area + 1e-8``; perspective
  correction with ``den = max(sum, 1e-8)``; clipped barycentrics renormalised over ``max(sum, 1e-5)``; a pair is dropped when
  ``pz < 0``;
* squared distance to the three segments with a clamped ``t`` (a degenerate edge: the distance to its end point), order e01, e02, e12,
  minimum with ``<=``; ``inside`` = all three corrected barycentrics ``> 0``; candidate if inside or ``d < blur``;
* the K smallest by (depth, face id); ``sil = 1 - prod (1 - sigmoid(-sd / sigma))``, formed through a sum of ``logsigmoid(sd / sigma)``;
* the blurred bounding-box test is left out: the distance test implies it (deviation 4);
* faces that cross ``z_clip`` are cut differentiably in float64 from the float32 inputs (pytorch3d ``clip_faces``: crossing points
  interpolated in view space), so autograd gives the xy hand-back and the depth gradient of the cut edges' end points;
* the gradient is ``torch.autograd`` with ``t`` detached: only x and y of ``verts_ndc`` receive gradient, cut edges excepted.

Beside the silhouette and the gradient it classifies every discrete decision of a pixel as sure or unsure by its float64 margin
(``Image.unsure``, rules in ``_analyse`` and ``_kept_terms``): a float32 implementation may decide an unsure one the other way, so
such pixels are taken out of a comparison (and their upstream gradient set to zero), never given a looser bound.
"""
import numpy as np
import torch

SIGMA = 1e-4
BLUR = float(np.log(1.0 / 1e-4 - 1.0) * SIGMA)
Z_CLIP = 5e-4
K_EPS = 1e-8
TAU_Z = 1e-5   # relative depth gap under which the order of two candidates is not sure in float32 (about 80 float32 ulps)
TAU = 1e-5     # the same margin for the other thresholds: blur, face validity, closest edge
FLIP = 1e-8    # a closest-edge choice matters when taking the other edge moves more than this share of the largest gradient mass
PAIRS_PER_CHUNK = 1_200_000  # (pixel, face) pairs evaluated at once: ~45 float64 temporaries of that size stay under 1 GB

F64 = torch.float64


def pixel_centres(S):
    """NDC coordinate of output column (or row) 0 .. S-1: both axes are flipped."""
    i = torch.arange(S, dtype=F64)
    return -1.0 + (2.0 * (S - 1 - i) + 1.0) / S


def clip_mesh(v, faces, z_clip):
    """pytorch3d ``clip_faces`` for one mesh, differentiable in ``v`` (V, 3) float64.  A vertex is behind when ``z < z_clip``.  One
    behind (p1; p2, p3 in front, cyclic order kept): the front part is (p4, p2, p3) + (p4, p3, p5).  Two behind (p1 in front):
    (p1, p4, p5).  p4 / p5 lie where p1-p2 / p1-p3 cross the plane, interpolated in view space: with ``w = (z_a - z_c) / (z_a - z_b)``,
    ``xy = (xy_a z_a (1 - w) + xy_b z_b w) / z_c``.  The cut face's own row becomes a zero-area placeholder, the front parts follow
    at F ..., the new vertices at V ...  Returns (v_aug, faces_aug, src (X, 2), new (X, 3) or None)."""
    z = v[:, 2].detach().numpy()
    behind = z[faces] < z_clip
    nb = behind.sum(1)
    ids = np.nonzero((nb == 1) | (nb == 2))[0]
    if ids.size == 0 or not z_clip > 0.0:
        return v, faces, np.zeros((0, 2), np.int64), None
    V, src, new_f, f_aug = v.shape[0], [], [], faces.copy()
    for fi in ids:
        tri, bh = faces[fi], behind[fi]
        k = int(np.nonzero(bh)[0][0]) if nb[fi] == 1 else int(np.nonzero(~bh)[0][0])  # the isolated vertex
        p1, p2, p3 = int(tri[k]), int(tri[(k + 1) % 3]), int(tri[(k + 2) % 3])
        p4, p5 = V + len(src), V + len(src) + 1
        src += [(p1, p2), (p1, p3)]
        new_f += [[p4, p2, p3], [p4, p3, p5]] if nb[fi] == 1 else [[p1, p4, p5]]
        f_aug[fi] = tri[0]
    src = np.asarray(src, np.int64)
    a, b = v[src[:, 0]], v[src[:, 1]]
    w = (a[:, 2] - z_clip) / (a[:, 2] - b[:, 2])
    xy = (a[:, :2] * (a[:, 2] * (1.0 - w))[:, None] + b[:, :2] * (b[:, 2] * w)[:, None]) / z_clip
    new = torch.cat([xy, torch.full((src.shape[0], 1), z_clip, dtype=F64)], 1)
    return torch.cat([v, new]), np.concatenate([f_aug, np.asarray(new_f, faces.dtype)]), src, new


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _segment(px, py, a, b):
    """Squared distance of (px, py) to the segment a-b, the clamped parameter (held constant) and the closest point."""
    bax, bay = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    l2 = bax * bax + bay * bay
    deg = l2 <= K_EPS
    t = ((bax * (px - a[..., 0]) + bay * (py - a[..., 1])) / torch.where(deg, torch.ones_like(l2), l2)).clamp(0.0, 1.0)
    t = torch.where(deg, torch.ones_like(t), t).detach()  # a degenerate edge: its end point b
    qx, qy = a[..., 0] + t * bax, a[..., 1] + t * bay
    return (qx - px) ** 2 + (qy - py) ** 2, t, qx, qy


def _barycentrics(px, py, v0, v1, v2):
    """Perspective-corrected barycentrics (unclipped) and the interpolated depth of the clipped, renormalised ones."""
    area = _edge(v2[..., 0], v2[..., 1], v0[..., 0], v0[..., 1], v1[..., 0], v1[..., 1]) + K_EPS
    b0 = _edge(px, py, v1[..., 0], v1[..., 1], v2[..., 0], v2[..., 1]) / area
    b1 = _edge(px, py, v2[..., 0], v2[..., 1], v0[..., 0], v0[..., 1]) / area
    b2 = _edge(px, py, v0[..., 0], v0[..., 1], v1[..., 0], v1[..., 1]) / area
    w0, w1, w2 = b0 * v1[..., 2] * v2[..., 2], b1 * v0[..., 2] * v2[..., 2], b2 * v0[..., 2] * v1[..., 2]
    den = (w0 + w1 + w2).clamp_min(K_EPS)
    p = torch.stack([w0 / den, w1 / den, w2 / den], -1)
    c = p.clamp_min(0.0)
    c = c / c.sum(-1, keepdim=True).clamp_min(1e-5)
    pz = c[..., 0] * v0[..., 2] + c[..., 1] * v1[..., 2] + c[..., 2] * v2[..., 2]
    return p, pz


class Image:
    """One image of the restatement.  Per pixel (S, S): ``sil`` float64, ``count`` candidates, ``trunc`` (count > K), ``unsure``.
    Per kept record (R,): ``rec_pixel`` (flat pixel), ``rec_face`` (id in the clipped mesh), ``rec_a`` / ``rec_b`` (end points of its
    closest edge, ids in the clipped mesh), ``rec_c`` (the third vertex) and ``rec_near`` (the two smallest edge distances lie within
    ``TAU``), ``rec_d`` (unsigned squared distance), ``rec_p`` (its probability).  ``alpha`` (S, S) is the product of ``1 - p``, ``reach`` (S, S) the
    largest distance of a candidate, ``why`` (S, S) the rules that make a pixel unsure (bit r - 1 for rule r)."""

    def gradient(self, g):
        """(V, 3) float64 gradient of ``sum(g * sil)`` with respect to the float32 input vertices, and (X, 2) the xy gradient of the
        new vertices of cut faces (what a rasteriser hands to ``clip_faces``' backward)."""
        g = torch.as_tensor(np.asarray(g, np.float64)).reshape(-1)
        for t in (self._v, self._new):
            if t is not None:
                t.grad = None
        if self._sil_t.requires_grad:
            (g * self._sil_t).sum().backward(retain_graph=True)
        gv = np.zeros(tuple(self._v.shape)) if self._v.grad is None else self._v.grad.numpy().copy()
        gn = np.zeros((self.src.shape[0], 2))
        if self._new is not None and self._new.grad is not None:
            gn = self._new.grad.numpy()[:, :2].copy()
        return gv, gn

    def touched(self, g):
        """(V,) bool: input vertices that a kept record of a pixel with ``g != 0`` reaches (through a cut edge's end points too)."""
        live = (np.asarray(g).reshape(-1) != 0)[self.rec_pixel]
        t = np.zeros(self.V + self.src.shape[0], bool)
        t[self.rec_a[live]] = True
        t[self.rec_b[live]] = True
        t[self.rec_c[live & self.rec_near]] = True  # (a near-tie of the closest edge too small to count as unsure: the other edge's end point)
        for j in np.nonzero(t[self.V:])[0]:
            t[self.src[j]] = True
        return t[:self.V]

    def accumulator_term(self, g, quantum=None, tile=8):
        """(V, 2) the absolute error the kernel's fixed-point gradient sums may add to a vertex component: half a quantum per kept
        record that reaches the component.  ``quantum``: the fixed-point unit of a packed launch (the decode factor the
        engine returns); None: the unit of each 8 x 8 tile, ``2^(floor(log2 bound) - 29)`` - the power of two that maps ``bound`` into
        [2^29, 2^30) - with ``bound = 2 r_max sum |coef_pixel|`` over the tile, ``|coef| = |g| alpha / sigma`` and ``r_max`` the largest
        distance of a candidate of the tile, kept or not (a tile dealt out in pieces, a record or a pixel the kernel leaves out only make the
        bound smaller)."""
        S = self.S
        g = np.abs(np.asarray(g, np.float64)).reshape(S, S)
        coef = (g * self.alpha / self.sigma).reshape(-1)
        live = coef[self.rec_pixel] != 0
        py, px = self.rec_pixel // S, self.rec_pixel % S
        nt = (S + tile - 1) // tile
        tid = (py // tile) * nt + px // tile
        if quantum is None:
            rmax, csum = np.zeros(nt * nt), np.zeros(nt * nt)
            pp = np.arange(S * S)
            ptile = ((pp // S) // tile) * nt + (pp % S) // tile
            np.maximum.at(rmax, ptile, self.reach.reshape(-1))
            np.add.at(csum, ptile, coef)
            bound = 2.0 * rmax * csum
            q_rec = np.where(bound > 0, 2.0 ** (np.floor(np.log2(np.maximum(bound, 1e-300))) - 29.0), 0.0)[tid]
        else:
            q_rec = np.full(tid.shape, float(quantum))
        acc = np.zeros(self.V + self.src.shape[0])
        np.add.at(acc, self.rec_a[live], 0.5 * q_rec[live])
        np.add.at(acc, self.rec_b[live], 0.5 * q_rec[live])
        out = acc[:self.V].copy()
        for j in range(self.src.shape[0]):  # a new vertex hands back through |coefficients| that sum to at most |c_a| + |c_b|
            out[self.src[j]] += np.abs(self.clip_coef[j]) * acc[self.V + j]
        return np.repeat(out[:, None], 2, 1)


def render(verts, faces, S, K=100, blur=BLUR, sigma=SIGMA, z_clip=Z_CLIP):
    """``verts`` (V, 3) float32 (x_ndc, y_ndc, z_view), ``faces`` (F, 3) int -> ``Image``.  (float64 vertices are taken as they are:
    the steps of a finite difference.)"""
    verts = np.asarray(verts)
    assert verts.dtype in (np.float32, np.float64) and verts.ndim == 2
    faces = np.asarray(faces, np.int64)
    v = torch.from_numpy(verts.astype(np.float64)).requires_grad_()
    va, fa, src, new = clip_mesh(v, faces, z_clip)
    if new is not None:
        new.retain_grad()
    img = Image()
    img.S, img.K, img.V, img.sigma, img.src, img._v, img._new = S, K, verts.shape[0], sigma, src, v, new
    img.faces_aug = fa
    if src.shape[0]:
        a, b = v.detach()[src[:, 0]], v.detach()[src[:, 1]]
        w = (a[:, 2] - z_clip) / (a[:, 2] - b[:, 2])
        img.clip_coef = torch.stack([a[:, 2] * (1 - w) / z_clip, b[:, 2] * w / z_clip], 1).numpy()
    else:
        img.clip_coef = np.zeros((0, 2))
    with torch.no_grad():
        kept_pix, kept_face, count, unsure, reach = _analyse(va.detach(), fa, S, K, blur, z_clip)
    _kept_terms(img, va, fa, kept_pix, kept_face, unsure, S, blur, sigma)
    img.count = count.reshape(S, S).numpy()
    img.reach = reach.reshape(S, S).numpy()
    img.trunc = img.count > K
    img.why = unsure.reshape(S, S).numpy()  # which rule: bit r - 1 for rule r
    img.unsure = img.why != 0
    return img


def _analyse(va, fa, S, K, blur, z_clip):
    """Every (pixel, face) pair: the candidates, the K nearest by (depth, face id) and the sure / unsure rules that need all pairs.

    unsure, rule 1 (truncation): the pixel has more than K candidates, the first dropped one lies within ``TAU_Z`` (relative) of the
    last kept one's depth, and the candidates within that margin do not tie structurally.  A structural tie - cut by face id in any
    precision - is a group of bit-equal depths in which every member's clipped barycentrics are one-hot (two corrected barycentrics
    below ``-TAU``: the depth is a vertex's own), or in which all members have bit-equal vertex coordinates (twins).
    rule 2 (blur): a pair that is not inside has ``|d - blur| < TAU blur``.
    rule 3 (validity): a face whose ``zmin``, ``zmax`` or ``|area|`` lies within ``TAU`` (relative) of its threshold would be (or is)
    a candidate of the pixel."""
    f = torch.from_numpy(fa)
    tri = va[f]                                   # (F, 3, 3)
    zmin, zmax = tri[..., 2].min(1).values, tri[..., 2].max(1).values
    area = _edge(tri[:, 0, 0], tri[:, 0, 1], tri[:, 1, 0], tri[:, 1, 1], tri[:, 2, 0], tri[:, 2, 1])
    valid = ~((zmin < K_EPS) | (zmax < z_clip) | (area.abs() <= K_EPS))
    near = lambda x, thr: (x - thr).abs() < TAU * thr  # noqa: E731
    border = near(zmin, K_EPS) | near(zmax, z_clip) | near(area.abs(), K_EPS)
    use = torch.nonzero(valid | border)[:, 0]     # ascending: the face id order survives
    tri, valid_u, border_u = tri[use], valid[use], border[use]
    # twins: faces with bit-equal vertex coordinates share a class
    _, cls = np.unique(tri.reshape(-1, 9).numpy(), axis=0, return_inverse=True)
    cls = torch.from_numpy(cls.reshape(-1))
    Fu = use.shape[0]
    c = pixel_centres(S)
    count = torch.zeros(S * S, dtype=torch.int64)
    unsure = torch.zeros(S * S, dtype=torch.uint8)  # bit r - 1: rule r
    kept_pix, kept_face = [], []
    reach = torch.zeros(S * S, dtype=F64)  # the largest distance of a candidate, kept or not
    if Fu == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), count, unsure, reach
    rows = max(1, PAIRS_PER_CHUNK // (S * Fu))
    v0, v1, v2 = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    for y0 in range(0, S, rows):
        y1 = min(S, y0 + rows)
        py = c[y0:y1].repeat_interleave(S)[:, None]
        px = c.repeat(y1 - y0)[:, None]
        pix = torch.arange(y0 * S, y1 * S)
        p, pz = _barycentrics(px, py, v0, v1, v2)
        d = torch.minimum(torch.minimum(_segment(px, py, v0, v1)[0], _segment(px, py, v0, v2)[0]), _segment(px, py, v1, v2)[0])
        inside = (p > 0).all(-1)
        geo = (inside | (d < blur)) & ~(pz < 0)
        cand = geo & valid_u[None]
        unsure[pix] |= 4 * (geo & border_u[None]).any(1).to(torch.uint8)                                             # rule 3
        unsure[pix] |= 2 * (valid_u[None] & ~inside & ~(pz < 0) & ((d - blur).abs() < TAU * blur)).any(1).to(torch.uint8)  # rule 2
        n = cand.sum(1)
        count[pix] = n
        reach[pix] = torch.where(cand, d, torch.zeros_like(d)).amax(1).sqrt()
        zs, idx = torch.sort(torch.where(cand, pz, torch.full_like(pz, float("inf"))), dim=1, stable=True)
        kk = min(K, Fu)
        ok = torch.arange(kk)[None] < n[:, None]
        kept_pix.append(pix[:, None].expand(-1, kk)[ok])
        kept_face.append(use[idx[:, :kk]][ok])
        r = torch.nonzero(n > K)[:, 0]
        if r.numel():                                                                               # rule 1
            zs_r, idx_r = zs[r], idx[r]
            zb = zs_r[:, K - 1:K]
            grp = (zs_r - zb).abs() < TAU_Z * zb
            onehot = ((p[r] < -TAU).sum(-1) == 2).gather(1, idx_r)
            eq = zs_r == zb
            twin = cls[idx_r] == cls[idx_r[:, K - 1:K]]
            structural = (~grp | (onehot & eq)).all(1) | (~grp | (twin & eq)).all(1)
            unsure[pix[r]] |= (grp[:, K] & ~structural).to(torch.uint8)
    return torch.cat(kept_pix), torch.cat(kept_face), count, unsure, reach


def _kept_terms(img, va, fa, kept_pix, kept_face, unsure, S, blur, sigma):
    """The kept records once more, differentiably: distance, closest edge, blend.

    unsure, rule 4 (closest edge): the two smallest edge distances of a kept record differ by less than ``TAU`` (relative) while their
    closest points differ, so that the gradient would go to other vertices.  Next to a vertex that two edges share the two closest
    points meet and the two choices hand the vertices the same in the limit, so "differ" is measured by what it is about: the
    largest change, over the face's six vertex components, of what the record hands back per unit of upstream gradient when the
    other edge is taken, against ``FLIP`` of the image's largest sum of absolute hand-backs to one vertex component."""
    c = pixel_centres(S)
    px, py = c[kept_pix % S], c[kept_pix // S]
    ids = torch.from_numpy(fa)[kept_face]          # (R, 3)
    v0, v1, v2 = va[ids[:, 0]], va[ids[:, 1]], va[ids[:, 2]]
    seg = [_segment(px, py, v0, v1), _segment(px, py, v0, v2), _segment(px, py, v1, v2)]
    ds = torch.stack([s[0] for s in seg], 1)
    edge = torch.argmin(ds.detach(), 1)            # the first of equal minima: e01, e02, e12 with <=
    d = ds.gather(1, edge[:, None])[:, 0]
    with torch.no_grad():
        p, _ = _barycentrics(px, py, v0, v1, v2)
        inside = (p > 0).all(-1)
    sd = torch.where(inside, -d, d)
    logs = torch.nn.functional.logsigmoid(sd / sigma)   # log(1 - p), p = sigmoid(-sd / sigma)
    L = torch.zeros(S * S, dtype=F64).index_add(0, kept_pix, logs)
    img._sil_t = -torch.expm1(L)
    img.sil = img._sil_t.detach().reshape(S, S).numpy().copy()
    img.alpha = torch.exp(L.detach()).reshape(S, S).numpy()
    with torch.no_grad():                          # rule 4
        # what a record hands to its face's three vertices per unit of upstream gradient, for each edge that could be the closest
        R = kept_pix.shape[0]
        w = (torch.exp(L)[kept_pix] * torch.sigmoid(-sd / sigma) / sigma)[:, None, None]
        hand = torch.zeros(3, R, 3, 2, dtype=F64)  # [edge][record][vertex of the face][x, y]
        for e, (ia, ib) in enumerate(((0, 1), (0, 2), (1, 2))):
            r2 = 2.0 * torch.stack([seg[e][2] - px, seg[e][3] - py], 1)
            hand[e, :, ia] = r2 * (1.0 - seg[e][1])[:, None]
            hand[e, :, ib] = r2 * seg[e][1][:, None]
        hand = hand * w
        srt, order = torch.sort(ds, dim=1, stable=True)
        ar = torch.arange(R)
        mass = torch.zeros(va.shape[0], 2, dtype=F64).index_add(0, ids.reshape(-1), hand[order[:, 0], ar].abs().reshape(-1, 2))
        flip = (hand[order[:, 0], ar] - hand[order[:, 1], ar]).abs().amax((1, 2))
        near = (srt[:, 1] - srt[:, 0]) < TAU * srt[:, 1]
        unsure[kept_pix[near & (flip > FLIP * mass.max())]] |= 8
    ea = torch.tensor([0, 0, 1])[edge]
    eb = torch.tensor([1, 2, 2])[edge]
    img.rec_pixel, img.rec_face = kept_pix.numpy(), kept_face.numpy()
    img.rec_a = ids.gather(1, ea[:, None])[:, 0].numpy()
    img.rec_b = ids.gather(1, eb[:, None])[:, 0].numpy()
    img.rec_c = ids.gather(1, torch.tensor([2, 1, 0])[edge][:, None])[:, 0].numpy()  # the face's third vertex ...
    img.rec_near = near.numpy()                                                      # ... which a near-tie of the closest edge may reach
    img.rec_d = d.detach().numpy()
    img.rec_p = torch.sigmoid(-sd.detach() / sigma).numpy()
