"""Inputs shared by the CPU and GPU tests of the winding numbers: hand meshes with exact answers, the meshes the sign must survive
(an icosphere, the atta worker scan, a degenerate soup, the hull mesh of a small carve) and seeded clouds on, near and around them."""
import functools
import os

import numpy as np

import hull_mesh_ref as MR
import point_mesh_cases as PC
import winding_ref as WR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND = 0.05  # no generated point has a float64 winding number within this of 0.5: its side is not a question of rounding
NEAR, BOX, ON = 2000, 1000, 200
K_RANGE = (-14, -2)  # offsets along the normal: +-E 2^k, k uniform in this range
DECIDED_FROM = 2.0 ** -14  # ... and the decision is asserted for every point at least this (times E) from the surface

OCTANT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]  # seen from the origin: 1/8 of the sphere, normal away from it


def cube(lo=-1.0, hi=1.0, flip=False, top=True):
    """The cube [lo, hi]^3 as 12 faces oriented outwards (``flip``: inwards); ``top`` False: without the two faces at z = hi."""
    v = np.asarray([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float32)
    f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    f = np.asarray(f if top else f[:2] + f[4:], np.int64)
    return v, (f[:, ::-1].copy() if flip else f)


def nested_cubes():
    (v1, f1), (v2, f2) = cube(-1.0, 1.0), cube(-0.5, 0.5)
    return np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)])


@functools.lru_cache(maxsize=None)
def icosphere(level: int = 3):
    """The unit icosphere, 20 4^level faces (1 280 at level 3), oriented outwards; float32 vertices."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = out
    return np.asarray(v, np.float64).astype(np.float32), np.asarray(f, np.int64)


@functools.lru_cache(maxsize=1)
def atta():
    """The atta worker scan (10 878 faces; nearly closed, self-intersecting), centred and scaled to [-1, 1]."""
    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    v = d["verts"].astype(np.float64)
    v = v - v.mean(0)
    return (v / np.abs(v).max()).astype(np.float32), d["faces"].astype(np.int64)


def soup():
    return PC.random_mesh(71, 60, 2 * PC.TILE + 9, degenerate=True)


# ---- the small carve --------------------------------------------------------------------------------------------------------------
HULL_G, HULL_ORIGIN, HULL_VOXEL = 12, (-1.5, 0.25, -0.75), 0.125  # a ball of radius 4.6 voxels on a 12^3 lattice, dyadic placement


def hull_occupancy():
    return MR.ball(HULL_G, 4.6)  # (1,G,G,G) uint8


def hull_centres():
    """The voxel centres (G^3,3) float32 in the order of ``hull_occupancy().reshape(-1)`` (z, y, x: x fastest)."""
    c = np.arange(HULL_G) + 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return (np.asarray(HULL_ORIGIN)[None] + np.stack([x, y, z], -1).reshape(-1, 3) * HULL_VOXEL).astype(np.float32)


def hull_uniform_neighbourhood():
    """(G^3,) bool: the voxels whose 26 neighbours (outside the lattice: empty) share their occupancy."""
    occ = np.pad(hull_occupancy()[0].astype(np.int64), 1)
    G, same = HULL_G, np.ones((HULL_G,) * 3, bool)
    for dz in (0, 1, 2):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                same &= occ[dz:dz + G, dy:dy + G, dx:dx + G] == occ[1:-1, 1:-1, 1:-1]
    return same.reshape(-1)


@functools.lru_cache(maxsize=None)
def hull_mesh(taubin: int = 0):
    """The hull mesh of the small carve by the float64 restatement of the extraction, rounded once to float32."""
    m = MR.extract(hull_occupancy(), HULL_ORIGIN, HULL_VOXEL, MR.taubin_steps(taubin), want_normals=False)
    return m.verts.astype(np.float32), m.faces.astype(np.int64)


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
def _on_faces(rng, v, f, n):
    tri = v.astype(np.float64)[f[rng.integers(0, len(f), n)]]
    b = rng.uniform(0.05, 1.0, (n, 3))
    b /= b.sum(1, keepdims=True)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(normal, axis=1, keepdims=True)
    return (b[:, :, None] * tri).sum(1), np.where(length > 0, normal / np.where(length > 0, length, 1.0), 0.0)


def extent(verts, points=None):
    """E: the largest |coordinate| of the mesh (and the cloud)."""
    e = float(np.abs(np.asarray(verts, np.float64)).max())
    return e if points is None else max(e, float(np.abs(np.asarray(points, np.float64)).max()))


def cloud(verts, faces, seed, device=None):
    """NEAR points on random faces moved along the face's normal by +-E 2^k, k uniform in K_RANGE, then BOX points uniform in the
    bounding box: (NEAR + BOX, 3) float32.  Candidates whose float64 winding number lies within BAND of 0.5 are drawn again (one
    and a half times the counts are drawn and the first that qualify kept), so the side of every point is a fact about the mesh."""
    rng = np.random.default_rng(seed)
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    E = extent(v)
    n_near, n_box = NEAR * 3 // 2, BOX * 3 // 2
    on, normal = _on_faces(rng, v, f, n_near)
    k = rng.uniform(*K_RANGE, (n_near, 1))
    near = on + rng.choice([-1.0, 1.0], (n_near, 1)) * E * 2.0 ** k * normal
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    box = rng.uniform(lo, hi, (n_box, 3))
    out = []
    for cand, n in ((near, NEAR), (box, BOX)):
        cand = cand.astype(np.float32)
        keep = np.abs(WR.winding(v, f, cand, np.float64, device) - 0.5) >= 2 * BAND  # (twice: the band holds on any device's atan2)
        assert int(keep.sum()) >= n, (int(keep.sum()), n)
        out.append(cand[keep][:n])
    return np.concatenate(out)


def surface_cloud(verts, faces, seed):
    """ON points on random faces, the same at +E 2^-30 and at -E 2^-30 along the normal: (3 ON, 3) float32."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float32)
    on, normal = _on_faces(rng, v, np.asarray(faces, np.int64), ON)
    step = extent(v) * 2.0 ** -30 * normal
    return np.concatenate([on, on + step, on - step]).astype(np.float32)


# (name, mesh, seed): the decision and value sets; the icosphere also translated (float32 roundings grow with the offset)
def mesh_cases():
    v, f = icosphere()
    return [("icosphere", (v, f), 81), ("icosphere+3", ((v.astype(np.float64) + 3.0).astype(np.float32), f), 82),
            ("icosphere+100", ((v.astype(np.float64) + 100.0).astype(np.float32), f), 83), ("atta", atta(), 84), ("soup", soup(), 85),
            ("hull", hull_mesh(), 86)]


@functools.lru_cache(maxsize=None)
def case(name, device=None):
    """(verts, faces, points) of one of ``mesh_cases()``, built once per process."""
    _, (v, f), seed = next(c for c in mesh_cases() if c[0] == name)
    return v, f, cloud(v, f, seed, device)


NAMES = ("icosphere", "icosphere+3", "icosphere+100", "atta", "soup", "hull")
