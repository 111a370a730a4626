"""TEST INFRASTRUCTURE ONLY: the numpy float64 restatement of the hull's mesh extraction (surface nets on the lattice of voxel centres;
include/smilfit.h, "Hull meshes").  Never imported by the product.

Every floating-point step is written as the specification orders it - numpy evaluates an expression operation by operation, without
fused multiply-adds - so the kernel, which does the same operations in the same order with contraction off, differs by the one
rounding to float32 only.  The arrays are vectorised over the cubes of a frame; the ORDER of the sums is that of the loops below.

Names.  Sample (i, j, k) is inside iff ``occ != 0``; the lattice is padded by one layer of outside samples.  Cube (i, j, k), every index in
-1 .. G-1, spans samples i..i+1 x j..j+1 x k..k+1 and has the linear index (i+1) + (Gx+1)((j+1) + (Gy+1)(k+1)).  ``cfg`` of a cube: bit
dx + 2 dy + 4 dz is set iff corner sample (i+dx, j+dy, k+dz) is inside.
"""
from types import SimpleNamespace

import numpy as np

# the 12 edges of a cube in the specification's order: axis a = x, y, z; u = (a+1) % 3, v = (a+2) % 3; (ou, ov) = (0,0), (1,0), (0,1), (1,1)
EDGES = [(a, ou, ov) for a in range(3) for (ou, ov) in ((0, 0), (1, 0), (0, 1), (1, 1))]
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))  # the cube offsets (du, dv) around an edge, in cyclic order
# neighbours in the order -x, +x, -y, +y, -z, +z: (axis, step, the cfg bits of the shared face)
FACES6 = [(0, -1, 0x55), (0, 1, 0xAA), (1, -1, 0x33), (1, 1, 0xCC), (2, -1, 0x0F), (2, 1, 0xF0)]


def gibson_steps(n):
    return (0.5,) * int(n)


def taubin_steps(n):
    return (0.5, -0.53) * int(n)


def _bit(a, off_a, u, off_u, v, off_v):
    d = [0, 0, 0]
    d[a], d[u], d[v] = off_a, off_u, off_v
    return d[0] + 2 * d[1] + 4 * d[2]


def topology(occ_frame):
    """One frame (Gz,Gy,Gx) -> the mesh's integer side: ``ijk (V,3)`` the cube of every vertex (ascending cube index), ``cfg (V,)``, ``faces
    (F,3) int64``, ``vid`` the dense cube -> vertex grid (-1: none) indexed [k+1, j+1, i+1], and ``start (V,3)`` float64."""
    Gz, Gy, Gx = occ_frame.shape
    inside = np.zeros((Gz + 2, Gy + 2, Gx + 2), bool)
    inside[1:-1, 1:-1, 1:-1] = occ_frame != 0
    Cz, Cy, Cx = Gz + 1, Gy + 1, Gx + 1
    cfg = np.zeros((Cz, Cy, Cx), np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cfg |= inside[dz:dz + Cz, dy:dy + Cy, dx:dx + Cx].astype(np.int64) << (dx + 2 * dy + 4 * dz)
    active = (cfg != 0) & (cfg != 255)
    vid = np.where(active, np.cumsum(active.reshape(-1)).reshape(active.shape) - 1, -1)
    kk, jj, ii = np.nonzero(active)  # C order: ascending cube index
    ijk = np.stack([ii, jj, kk], 1).astype(np.int64) - 1
    c = cfg[kk, jj, ii]
    # start positions: the mean of the midpoints of the sign-changing edges (every summand a multiple of 0.5: the sum is exact)
    total = np.zeros((len(c), 3))
    count = np.zeros(len(c))
    for a, ou, ov in EDGES:
        u, v = (a + 1) % 3, (a + 2) % 3
        change = ((c >> _bit(a, 0, u, ou, v, ov)) & 1) != ((c >> _bit(a, 1, u, ou, v, ov)) & 1)
        mid = ijk.astype(np.float64)
        mid[:, a] += 0.5
        mid[:, u] += ou
        mid[:, v] += ov
        total = np.where(change[:, None], total + mid, total)
        count = count + change
    start = total / count[:, None] if len(c) else total
    # faces: the owned edges (from the minimum corner along +x, +y, +z) whose samples differ in kind
    quads, keys = [], []
    cube_index = (ii + Cx * (jj + Cy * kk)).astype(np.int64)
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        own = (c & 1) != ((c >> (1 << a)) & 1)
        pos = np.stack([ii, jj, kk], 1)[own]  # (x, y, z) + 1
        q = np.empty((len(pos), 4), np.int64)
        for m, (du, dv) in enumerate(QUAD):
            p = pos.copy()
            p[:, u] += du
            p[:, v] += dv
            q[:, m] = vid[p[:, 2], p[:, 1], p[:, 0]]
        assert (q >= 0).all()
        lower_outside = (c[own] & 1) == 0
        q = np.where(lower_outside[:, None], q[:, ::-1], q)
        quads.append(q)
        keys.append(cube_index[own] * 3 + a)
    quads, keys = np.concatenate(quads), np.concatenate(keys)
    quads = quads[np.argsort(keys, kind="stable")]
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return SimpleNamespace(ijk=ijk, cfg=c, faces=faces, vid=vid, start=start)


def _neighbour(top, axis, step):
    p = top.ijk + 1
    p[:, axis] += step
    ok = (p[:, axis] >= 0) & (p[:, axis] < top.vid.shape[2 - axis])
    p[:, axis] = np.clip(p[:, axis], 0, top.vid.shape[2 - axis] - 1)
    return np.where(ok, top.vid[p[:, 2], p[:, 1], p[:, 0]], -1)


def relax(top, weights):
    """The schedule's Jacobi steps on the index coordinates (V,3) float64."""
    pos = top.start.copy()
    if not len(pos):
        return pos
    lo, hi = top.ijk.astype(np.float64), top.ijk.astype(np.float64) + 1.0
    nbrs = []
    for axis, step, bits in FACES6:
        f = top.cfg & bits
        mixed = (f != 0) & (f != bits)
        n = _neighbour(top, axis, step)
        assert (n[mixed] >= 0).all()
        nbrs.append((mixed, np.where(mixed, n, 0)))
    for w in weights:
        total = np.zeros_like(pos)
        count = np.zeros(len(pos))
        for mixed, n in nbrs:
            total = np.where(mixed[:, None], total + pos[n], total)
            count = count + mixed
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mean = total / count[:, None]
            moved = pos + np.float64(w) * (mean - pos)
            moved = np.minimum(np.maximum(moved, lo), hi)
        pos = np.where((count > 0)[:, None], moved, pos)
    return pos


def world(pos, origin, voxel):
    """origin + (u + 0.5) * voxel, float64 (three roundings)."""
    return np.asarray(origin, np.float64)[None, :] + (pos + 0.5) * np.float64(voxel)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def normals(top, pos, voxel):
    """The area-weighted vertex normals as a gather, float64 (V,3)."""
    V = len(pos)
    out = np.zeros((V, 3))
    if not V:
        return out
    scaled = pos * np.float64(voxel)
    me = np.arange(V)
    for a, ou, ov in EDGES:
        u, v = (a + 1) % 3, (a + 2) % 3
        lower = (top.cfg >> _bit(a, 0, u, ou, v, ov)) & 1
        change = lower != ((top.cfg >> _bit(a, 1, u, ou, v, ov)) & 1)
        q = np.zeros((V, 4), np.int64)
        for m, (du, dv) in enumerate(QUAD):
            p = top.ijk + 1
            p[:, u] += ou + du
            p[:, v] += ov + dv
            inb = (p[:, u] >= 0) & (p[:, v] >= 0) & (p[:, u] < top.vid.shape[2 - u]) & (p[:, v] < top.vid.shape[2 - v])
            p = np.where(inb[:, None], p, 0)
            q[:, m] = np.where(change & inb, top.vid[p[:, 2], p[:, 1], p[:, 0]], 0)
            assert (q[change, m] >= 0).all() and inb[change].all()
        q = np.where((lower == 0)[:, None], q[:, ::-1], q)
        for tri in ((0, 1, 2), (0, 2, 3)):
            t = q[:, tri]
            holds = change & (t == me[:, None]).any(1)
            p0, p1, p2 = scaled[t[:, 0]], scaled[t[:, 1]], scaled[t[:, 2]]
            out = np.where(holds[:, None], out + _cross(p1 - p0, p2 - p0), out)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt(out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1] + out[:, 2] * out[:, 2])
        unit = out / length[:, None]
    return np.where((length == 0)[:, None], 0.0, unit)


def topologies(occ):
    return [topology(f) for f in occ]


def assemble(tops, positions, origin=(0.0, 0.0, 0.0), voxel=1.0, want_normals=True):
    """The packed mesh of the frames' ``topology`` and relaxed index coordinates (``relax``): see ``extract``."""
    N = len(tops)
    origin = np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 3), (N, 3))
    voxel = np.broadcast_to(np.asarray(voxel, np.float64).reshape(-1), (N,))
    verts = [world(pos, origin[n], voxel[n]) for n, pos in enumerate(positions)]
    norms = [normals(top, pos, voxel[n]) if want_normals else np.zeros_like(pos) for n, (top, pos) in enumerate(zip(tops, positions))]
    faces = [top.faces for top in tops]
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)  # noqa: E731
    return SimpleNamespace(verts=np.concatenate(verts), normals=np.concatenate(norms), index=np.concatenate(positions),
                           cubes=np.concatenate([top.ijk for top in tops]), faces=np.concatenate(faces).astype(np.int64), vert_offsets=off(verts),
                           face_offsets=off(faces))


def extract(occ, origin=(0.0, 0.0, 0.0), voxel=1.0, weights=(), want_normals=True, tops=None):
    """The packed mesh of ``occ (N,Gz,Gy,Gx)``: ``verts``, ``normals`` (Vt,3) float64 (round them once to float32 to compare), ``index``
    (Vt,3) the final index coordinates, ``cubes (Vt,3)``, ``faces (Ft,3)`` int64 frame-local, ``vert_offsets``, ``face_offsets`` (N+1) int64.
    ``origin`` (3,), (1,3) or (N,3), ``voxel`` a number, (1,) or (N,).  ``tops``: the frames' ``topology`` if already at hand."""
    tops = topologies(occ) if tops is None else tops
    return assemble(tops, [relax(top, weights) for top in tops], origin, voxel, want_normals)


def signed_volume(verts, faces):
    """The divergence theorem's sum over the triangles, float64."""
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float((a * _cross(b, c)).sum() / 6.0)


def ball(G=12, radius=4.6):
    """(1,G,G,G) uint8: the voxels whose centres lie within ``radius`` voxels of the grid's centre."""
    k, j, i = np.meshgrid(*(np.arange(G) - 0.5 * (G - 1),) * 3, indexing="ij")
    return ((i * i + j * j + k * k <= radius * radius).astype(np.uint8))[None]
