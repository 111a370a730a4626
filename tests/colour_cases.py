"""The generated scenes of the colour (HardPhong) edge tests, shared by the CPU test of their conditions (tests/test_colour_cpu.py) and
the GPU tests (tests/test_gpu_colour_edges.py): every scene is seeded, built once, judged once by the float64 restatement
(tests/shade_ref.py) and cached.  ``render_colour`` takes ``verts_ndc`` directly, so a scene may place its faces in NDC and view depth by
hand and still carry world vertices for the shading.  Vertices carry fixed irrational-looking offsets that keep them (and the edges
between them) off the pixel-centre lattice, so the restatement's ``unsure`` set stays small.

partial{S}        a sphere over the image's last row and column of tiles at S = 9, 17, 63, 65 (no multiple of the 8 x 8 tile).
overflow          128 large faces at S = 64: image 0 has more than twice the (tile, face) entries its lists may hold and is drawn
                  by the unbinned loop; image 1 (the same faces shrunk about the centre) is binned.
size520, size516  the sphere at S = 520 (65 x 65 tiles > COUNT_TILES_MAX: never binned) and S = 516 (the same, with partial tiles).
ties_*            face k + F/2 repeats face k (same vertex ids, same order): ``batch`` 48 entries on one tile, ``batches`` 160 (the
                  copies in different 64-entry batches), ``permuted`` the rows of ``batches`` shuffled (a tile's list holds the
                  even ids before the odd ones, so for many pairs the higher id is read first), ``overflow`` 64 + 64 large faces in
                  the unbinned loop (the copies in different 64-face groups).
stack{n}_{order}  one tile covered by exactly n = 64, 65, 128, 129 whole faces at depths 0.15 % apart, ids near to far or far to
                  near; stack129_partial: the nearest face covers only a corner of the tile, the others come far to near.
cuts              three images; face 0 has vertex c behind z_clip (two front parts), face 1 all but vertex c (one part), c = image;
                  a strip of four faces crossing the plane.
specular          a patch of a sphere of radius 2 whose mirror direction of the light at (0, 0, 3) passes through the camera.
backfacing        the same patch with every face turned over: n.d < 0 on every hit although v.r > 0.
degenerate        a vertex of no face, two faces without area, two pairs of faces of opposite orientation sharing an edge (the
                  interpolated normal is zero along that edge, respectively along a line inside the smaller face).
cameras_{N,1,views}  3 frames x 2 views of a sphere through camera tables of N = 6, 1 and 2 rows.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import shade_ref
from oracle import render_ref

RGB = [0.0, 172.0 / 255.0, 223.0 / 255.0]
TILE = 8
LIST_CAP_PER_FACE = 8      # list entries an image may have per face (doubled above S = 256)
COUNT_TILES_MAX = 4096     # images with more tiles are never binned
TAN30 = math.tan(math.radians(30.0))
O1, O2, O3 = math.sqrt(2.0) - 1.4, math.sqrt(3.0) - 1.7, math.sqrt(5.0) - 2.2   # 0.0142, 0.0321, 0.0361

PARTIAL_SIZES = [9, 17, 63, 65]
STACKS = [f"stack{n}_{o}" for n in (64, 65, 128, 129) for o in ("near", "far")] + ["stack129_partial"]
TIES = ["ties_batch", "ties_batches", "ties_permuted", "ties_overflow"]
SHADING = ["specular", "backfacing", "degenerate"]
CAMERAS = ["cameras_N", "cameras_1", "cameras_views"]
SCENES = ([f"partial{S}" for S in PARTIAL_SIZES] + ["overflow", "size520", "size516"] + TIES + STACKS + ["cuts"] + SHADING + CAMERAS)
STACK_TILE = (1, 1)        # (tx, ty) of the tile the stack scenes cover


def list_cap(F, S):
    """Entries the binned lists of one image may hold (0: the image is never binned): the rule of the setup kernel."""
    tiles_x = -(-S // TILE)
    return LIST_CAP_PER_FACE * (2 if S > 256 else 1) * F if tiles_x * tiles_x <= COUNT_TILES_MAX else 0


def ndc_of(u, S):
    """NDC of the continuous output coordinate ``u`` (pixel ``xo`` has its centre at u = xo)."""
    return -1.0 + (2.0 * (S - 1 - np.asarray(u, np.float64)) + 1.0) / S


def tile_entries(ndc, faces, S, slack=0.0):
    """(tiles, tiles) [ty, tx] numbers of faces whose tile box holds the tile, by the setup kernel's rule: the pixel centres inside the
    face's box, widened by ``slack`` pixels (the kernel: 0.01), in tile units.  For images without cut faces."""
    ndc = np.asarray(ndc, np.float64)
    tiles_x = -(-S // TILE)
    out = np.zeros((tiles_x, tiles_x), np.int64)
    for tri in np.asarray(faces):
        x, y, z = ndc[tri, 0], ndc[tri, 1], ndc[tri, 2]
        assert not (z < shade_ref.Z_CLIP).any()
        area = (x[2] - x[0]) * (y[1] - y[0]) - (y[2] - y[0]) * (x[1] - x[0])
        if z.min() < shade_ref.EPS or abs(area) <= shade_ref.EPS:
            continue
        v = lambda c: ((c + 1.0) * S - 1.0) * 0.5  # noqa: E731
        xi_lo, xi_hi = max(math.ceil(v(x.min()) - slack), 0), min(math.floor(v(x.max()) + slack), S - 1)
        yi_lo, yi_hi = max(math.ceil(v(y.min()) - slack), 0), min(math.floor(v(y.max()) + slack), S - 1)
        if xi_lo > xi_hi or yi_lo > yi_hi:
            continue
        out[(S - 1 - yi_hi) // TILE:(S - 1 - yi_lo) // TILE + 1, (S - 1 - xi_hi) // TILE:(S - 1 - xi_lo) // TILE + 1] += 1
    return out


# ----------------------------------------------------------------------------------------------
# building blocks
# ----------------------------------------------------------------------------------------------
def _default_camera():
    R, T = render_ref.look_at_view_transform(2.7, 0.0, 0.0)  # R = diag(-1, 1, -1), T = (0, 0, 2.7)
    return R.numpy().astype(np.float32), T.numpy().astype(np.float32)


def _world_of(ndc, scale=1.0):
    """World points that the default camera (fov 60) sends to ``ndc`` = (x_ndc, y_ndc, z_view), ``scale`` times as far away."""
    ndc = np.asarray(ndc, np.float64)
    z = ndc[..., 2]
    return np.stack([-ndc[..., 0] * z * TAN30 * scale, ndc[..., 1] * z * TAN30 * scale, 2.7 - z * scale], -1)


def _scene(name, world, ndc, faces, S, R=None, T=None, views=1, dup_of=None, fov=None, aspect=None, **info):
    if R is None:
        R, T = _default_camera()
    world, ndc = np.asarray(world, np.float32), np.asarray(ndc, np.float32)
    world = world[None] if world.ndim == 2 else world
    ndc = ndc[None] if ndc.ndim == 2 else ndc
    assert ndc.shape[0] == world.shape[0] * views
    return SimpleNamespace(name=name, verts_world=np.ascontiguousarray(world), verts_ndc=np.ascontiguousarray(ndc),
                           faces=np.ascontiguousarray(faces, dtype=np.int32), R=np.ascontiguousarray(R, dtype=np.float32),
                           T=np.ascontiguousarray(T, dtype=np.float32), S=S, views=views, N=ndc.shape[0], F=len(faces),
                           dup_of=dup_of, fov=np.asarray([60.0] if fov is None else fov, np.float32),
                           aspect=None if aspect is None else np.asarray(aspect, np.float32), info=info)


def _rotation(seed):
    q = np.random.default_rng(seed).normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _sphere(radius, centre, seed, nu=12, nv=8):
    """UV sphere of 2 nu (nv - 1) = 168 faces, outward orientation, turned by a seeded rotation."""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, nv):
        th = math.pi * i / nv
        for j in range(nu):
            ph = 2.0 * math.pi * (j + 0.5 * (i % 2)) / nu
            v.append([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
    v.append([0.0, 0.0, -1.0])
    ring = lambda i, j: 1 + (i - 1) * nu + j % nu  # noqa: E731
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(nu)]
    for i in range(1, nv - 1):
        for j in range(nu):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            f += [[a, c, d], [a, d, b]] if (i + j) % 2 else [[a, c, b], [b, c, d]]
    last = len(v) - 1
    f += [[last, ring(nv - 1, j + 1), ring(nv - 1, j)] for j in range(nu)]
    v = np.asarray(v) @ _rotation(seed).T * radius + np.asarray(centre)
    return v, np.asarray(f)


def _project(world, R, T, fov, aspect=None):
    """(N,V,3) float32 NDC of ``world`` (frames,V,3) through per-image cameras (image n = frame * views + view)."""
    R, T = torch.from_numpy(np.asarray(R, np.float32)), torch.from_numpy(np.asarray(T, np.float32))
    n = R.shape[0]
    pts = torch.from_numpy(np.asarray(world, np.float32))
    pts = pts.repeat_interleave(n // pts.shape[0], 0)
    asp = None if aspect is None else torch.from_numpy(np.asarray(aspect, np.float32))
    return render_ref.project_to_ndc(pts, R, T, torch.from_numpy(np.asarray(fov, np.float32)), asp).numpy()


def _corner_sphere(name, S):
    v, f = _sphere(0.9, [0.85 + O1, -0.8 + O2, O3], seed=11)
    R, T = _default_camera()
    return _scene(name, v, _project(v[None], R, T, [60.0]), f, S)


def _stack(name, n, order, tilt=0.0, copies=False, permute=False, seed=5, S=32):
    """n right triangles over tile (1, 1) of a 32 x 32 image, each covering all 64 of its pixels and reaching into tiles 1..2 only
    (4 list entries each, so the image stays binned); rank r lies at depth 1.0015^r.  ``tilt``: per-vertex depths in [1, 1 + tilt]
    instead, so that the nearest face changes from pixel to pixel.  ``copies``: the table repeats itself."""
    rng = np.random.default_rng(seed)
    partial = order == "partial"
    uv, z = np.zeros((n, 3, 2)), np.zeros((n, 3))
    for k in range(n):
        rank = k if order == "near" else n - 1 - k
        u0, v0, L = 7.3 + O1 + rng.uniform(-0.2, 0.2), 7.3 + O2 + rng.uniform(-0.2, 0.2), 16.1 + rng.uniform(-0.2, 0.2)
        if partial and k == 0:  # the nearest face: a corner of the tile only
            rank, L = -40, 6.3 + O3
        tri = np.array([[u0, v0], [u0 + L, v0], [u0, v0 + L]])
        uv[k] = tri if k % 2 else tri[::-1]  # (both orientations)
        z[k] = rng.uniform(1.0, 1.0 + tilt, 3) if tilt else 1.0015 ** rank * (1.0 + 2e-4 * np.array([-1.0, 0.0, 1.0]))
    ndc = np.concatenate([ndc_of(uv, S), z[..., None]], -1).reshape(3 * n, 3)
    faces = np.arange(3 * n).reshape(n, 3)
    dup_of = None
    if copies:
        faces = np.concatenate([faces, faces])
        dup_of = np.concatenate([np.arange(n), np.arange(n)])
        if permute:
            perm = np.random.default_rng(seed + 1).permutation(2 * n)
            faces, key = faces[perm], dup_of[perm]
            dup_of = np.array([int(np.nonzero(key == k)[0].min()) for k in key])
    return _scene(name, _world_of(ndc), ndc, faces, S, dup_of=dup_of)


def _large_faces(name, n, copies, seed, S=64):
    """n triangles whose boxes cover at least 20 of the 64 tiles each (image 0) and the same shrunk about the centre (image 1)."""
    rng = np.random.default_rng(seed)
    uv = np.zeros((n, 3, 2))
    k = 0
    while k < n:
        tri = rng.uniform(-4.0, S + 3.0, (3, 2)) + [O1, O2]
        ext = np.clip(tri.max(0), 0, S - 1) // TILE - np.clip(tri.min(0), 0, S - 1) // TILE
        a = (tri[2, 0] - tri[0, 0]) * (tri[1, 1] - tri[0, 1]) - (tri[2, 1] - tri[0, 1]) * (tri[1, 0] - tri[0, 0])
        if ext.min() >= 4 and abs(a) > 0.15 * S * S:
            uv[k] = tri
            k += 1
    z = rng.uniform(1.0, 2.0, (n, 3, 1))
    big = np.concatenate([ndc_of(uv, S), z], -1).reshape(3 * n, 3)
    small = np.concatenate([ndc_of((S - 1) / 2 + O3 + 0.15 * (uv - (S - 1) / 2), S), z], -1).reshape(3 * n, 3)
    faces = np.arange(3 * n).reshape(n, 3)
    dup_of = None
    if copies:
        faces, dup_of = np.concatenate([faces, faces]), np.concatenate([np.arange(n), np.arange(n)])
    ndc = np.stack([big, small])
    return _scene(name, _world_of(ndc), ndc, faces, S, dup_of=dup_of)


def _cuts(name, S=48):
    """Faces of a few millimetres around a camera at the origin of view space, given as view points (x, y, z): NDC = (x, y) / (z tan 30).
    Image c: vertex c of face 0 is the one behind the plane, vertex c of face 1 the one in front.  The world vertices are the view
    points 250 times as far away (default camera), so that position and shading vary visibly over a face."""
    one = np.array([[0.0003, 0.0002, -0.003], [-0.001, 0.0045, 0.012], [-0.0045, -0.002, 0.010]])   # roles: behind, front, front
    two = np.array([[0.0005, 0.001, 0.011], [0.0002, 0.0006, -0.004], [0.0005, -0.0004, -0.002]])   # roles: front, behind, behind
    strip = np.array([[-0.004 + 0.004 * i, -0.0045, 0.009] for i in range(3)] + [[-0.0038 + 0.004 * i, -0.004, -0.002] for i in range(3)])
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 9], [7, 10, 9], [7, 8, 10], [8, 11, 10]])
    view = np.zeros((3, 12, 3))
    for c in range(3):
        for r in range(3):  # role r goes to corner (c + r) % 3: the cyclic order, hence the orientation, is kept
            view[c, (c + r) % 3] = one[r]
            view[c, 3 + (c + r) % 3] = two[r]
        view[c, 6:] = strip
        view[c, :, :2] += 1e-5 * np.array([O1, O2]) * (1 + c)
    ndc = np.concatenate([view[..., :2] / (view[..., 2:] * TAN30), view[..., 2:]], -1)
    behind = (view[0][faces][..., 2] < shade_ref.Z_CLIP).sum(1)
    return _scene(name, _world_of(ndc, scale=250.0), ndc, faces, S, n_behind=behind)


def _patch(name, flip, S=64, n=8):
    """(n + 1)^2 vertices of the sphere of radius 2 about (0, 0, -1), over |x|, |y| <= 0.62 around its pole (0, 0, 1): the light at
    (0, 0, 3) and the default camera at (0, 0, 2.7) both stand over the pole."""
    g = np.linspace(-0.62, 0.62, n + 1)
    x, y = np.meshgrid(g + 0.05 + O1, g - 0.03 + O2, indexing="xy")
    v = np.stack([x, y, np.sqrt(4.0 - x * x - y * y) - 1.0], -1).reshape(-1, 3)
    f = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1
            f += [[a, b, d], [a, d, c]] if (i + j) % 2 else [[a, b, c], [b, d, c]]
    f = np.asarray(f)
    R, T = _default_camera()
    return _scene(name, v, _project(v[None], R, T, [60.0]), f[:, ::-1] if flip else f, S)


def _degenerate(name, S=50):
    """World coordinates are multiples of 1/8 in two tilted planes and NDC x, y = 0.75 world + const are multiples of 1/256, so that in
    float32 as in float64 the faces without area have exactly none and the opposite normals cancel exactly."""
    xy = np.array([[-0.5, -0.5], [-0.5, 0.25], [-0.125, -0.125], [-0.875, -0.125],     # 0-3: a, b, c, d: (a,b,c) and (a,b,d), equal areas
                   [0.5, -0.875],                                                         # 4: a vertex of no face
                   [0.25, -0.5], [0.25, 0.5], [0.875, 0.0], [0.0, 0.0],                   # 5-8: e, f, g, h: (e,f,g) large, (e,f,h) small
                   [0.25, 0.0],                                                           # 9: on the edge e-f, only in the face without area
                   [-0.375, 0.5], [0.125, 0.5], [0.125, 0.875], [-0.375, 0.875]])         # 10-13: an ordinary quadrilateral
    wz = np.where(np.arange(len(xy)) < 5, 0.25 * xy[:, 0] + 0.125 * xy[:, 1], -0.125 * xy[:, 0] + 0.25 * xy[:, 1])
    wz[10:] = [0.0, 0.125, 0.0, 0.25]
    world = np.concatenate([xy, wz[:, None]], -1)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 0, 1], [5, 6, 7], [5, 6, 8], [5, 9, 6], [10, 11, 12], [10, 12, 13]])
    ndc = np.concatenate([0.75 * xy + [3.0 / 256.0, -5.0 / 256.0], 2.7 - wz[:, None]], -1)
    return _scene(name, world, ndc, faces, S, no_area=[2, 5], unused_vertex=4)


def _cameras(name, rows, S=64):
    frames, views = 3, 2
    N = frames * views
    world = np.stack([_sphere(0.8, [0.1 * k + O1, -0.08 * k + O2, 0.15 * k], seed=20 + k)[0] for k in range(frames)])
    faces = _sphere(0.8, [0, 0, 0], seed=0)[1]
    R, T = render_ref.look_at_view_transform(torch.tensor([2.5, 2.7, 2.9, 2.6, 2.8, 3.0]), torch.linspace(-10, 25, N), torch.linspace(-30, 40, N))
    fov, aspect = np.linspace(45.0, 70.0, N), np.linspace(0.9, 1.3, N)
    R, T, fov, aspect = R.numpy()[:rows], T.numpy()[:rows], fov[:rows], aspect[:rows]
    idx = np.arange(N) % rows
    return _scene(name, world, _project(world, R[idx], T[idx], fov[idx], aspect[idx]), faces, S, R=R, T=T, views=views, fov=fov, aspect=aspect)


@functools.lru_cache(maxsize=None)
def get(name):
    if name.startswith("partial"):
        return _corner_sphere(name, int(name[7:]))
    if name.startswith("size"):
        return _corner_sphere(name, int(name[4:]))
    if name == "overflow":
        return _large_faces(name, 128, False, seed=2)
    if name == "ties_overflow":
        return _large_faces(name, 64, True, seed=3)
    if name == "ties_batch":
        return _stack(name, 24, "near", tilt=0.5, copies=True)
    if name in ("ties_batches", "ties_permuted"):
        return _stack(name, 80, "near", tilt=0.5, copies=True, permute=name == "ties_permuted")
    if name.startswith("stack"):
        n, order = name[5:].split("_")
        return _stack(name, int(n), order, seed=int(n))
    if name == "cuts":
        return _cuts(name)
    if name in ("specular", "backfacing"):
        return _patch(name, flip=name == "backfacing")
    if name == "degenerate":
        return _degenerate(name)
    if name.startswith("cameras_"):
        return _cameras(name, {"N": 6, "1": 1, "views": 2}[name[8:]])
    raise KeyError(name)


# ----------------------------------------------------------------------------------------------
# the restatement's answer, once per scene
# ----------------------------------------------------------------------------------------------
NLEN_MIN = 1e-4   # declared exclusion (colour only): the interpolated normal is shorter than this before it is normalised, so the sign of
                  # n.d, or the clamp at 1e-6, hangs on the last bits of the barycentrics


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per image of the scene a namespace: ``image`` (3,S,S) float64, ``image32`` the same formulas in float32 from float32 inputs at
    the same barycentrics, the arrays of ``shade_ref.raster_k1_detail`` as attributes, the per-hit ``terms`` of
    ``shade_ref.shade_terms`` and ``excluded`` (S,S), the declared colour exclusions."""
    s = get(name)
    out = []
    for n in range(s.N):
        d = shade_ref.raster_k1_detail(s.verts_ndc[n].astype(np.float64), s.faces, s.S, dup_of=s.dup_of)
        vw, R, T = s.verts_world[n // s.views], s.R[n % len(s.R)], s.T[n % len(s.T)]
        p2f, bary = d["pix_to_face"], d["bary"]
        terms = shade_ref.shade_terms(p2f, bary, vw, s.faces, R, T) if (p2f >= 0).any() else None
        excluded = np.zeros((s.S, s.S), bool)
        if terms is not None:
            excluded[p2f >= 0] = terms["nlen"] < NLEN_MIN
        out.append(SimpleNamespace(image=shade_ref.shade(p2f, bary, vw, s.faces, R, T, RGB),
                                   image32=shade_ref.shade(p2f, bary, vw, s.faces, R, T, RGB, dtype=np.float32),
                                   terms=terms, excluded=excluded, **d))
    return out


def compare_image(img, p2f, ref_img, ref_p2f, unsure, F, unsure_face=None, excluded=None):
    """One rendered image (3,S,S), (S,S) against the restatement: no ``pix_to_face`` mismatch outside ``unsure_face`` (default:
    ``unsure``), ids in range, colour within 2e-4 wherever both name the same face (but for ``excluded``), background exactly 1.
    Returns ``(mismatches inside unsure, compared hit pixels, largest colour error, compared mask)``."""
    diff = p2f != ref_p2f
    loose = unsure if unsure_face is None else unsure_face
    assert not (diff & ~loose).any(), (np.argwhere(diff & ~loose)[:8], p2f[diff & ~loose][:8], ref_p2f[diff & ~loose][:8])
    assert p2f.max() < F and p2f.min() >= -1
    agree = ~diff & (ref_p2f >= 0)
    if excluded is not None:
        agree &= ~excluded
    err = float(np.abs(img[:, agree] - ref_img[:, agree]).max()) if agree.any() else 0.0
    assert err <= 2e-4, err
    bg = (ref_p2f < 0) & (p2f < 0)
    assert (img[:, bg] == 1.0).all()
    assert (img[:, p2f < 0] == 1.0).all()
    return int(diff.sum()), int(agree.sum()), err, agree
