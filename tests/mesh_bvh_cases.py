"""Inputs shared by the CPU and GPU tests of the mesh hierarchy (csrc/mesh_bvh.hip): the shapes at which a tree can go wrong where the
brute force cannot - every distance a tie, every code equal, face counts around a leaf, clusters far apart.  The generators of
tests/point_mesh_cases.py cover the rest."""
import numpy as np

import point_mesh_cases as PC


def leaf_size() -> int:
    from smilify_amd import _lib

    return int(_lib.BVH_LEAF)  # SMIL_BVH_LEAF of include/smilfit.h


def face_counts():
    """0 and 1, around one leaf, around 128 (2^k leaves and one more) and many levels."""
    leaf = leaf_size()
    return [0, 1, leaf - 1, leaf, leaf + 1, 127, 128, 129, 1000]


POINT_COUNTS = (1, 255, 256, 257)


def copies(n: int = 300):
    """n copies of one triangle over three shared vertices: every Morton code is equal and every distance is an n-fold tie."""
    verts = np.asarray(PC.TRI, np.float32)
    return verts, np.tile(np.arange(3, dtype=np.int64), (n, 1))


def lattice(n: int = 32):
    """A planar mesh of n x n unit quads, two faces each, and its queries: the (n+1)^2 lattice points, the cell centres (on a
    diagonal: two faces) and the edge mid-points - every answer is d^2 = 0 on two to six faces."""
    g = np.arange(n + 1, dtype=np.float32)
    x, y = np.meshgrid(g, g, indexing="xy")
    verts = np.stack([x.ravel(), y.ravel(), np.zeros((n + 1) ** 2, np.float32)], 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    a = (j * (n + 1) + i).ravel()
    faces = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)]).astype(np.int64)
    c = np.stack([(x[:-1, :-1] + 0.5).ravel(), (y[:-1, :-1] + 0.5).ravel(), np.zeros(n * n, np.float32)], 1)
    ex = np.stack([(x[:, :-1] + 0.5).ravel(), y[:, :-1].ravel(), np.zeros(n * (n + 1), np.float32)], 1)
    ey = np.stack([x[:-1, :].ravel(), (y[:-1, :] + 0.5).ravel(), np.zeros(n * (n + 1), np.float32)], 1)
    return verts, faces, np.concatenate([verts, c, ex, ey]).astype(np.float32)


def hull_occupancy(G: int = 12):
    """(1, G, G, G) uint8: a ball, and beside it two voxels that touch along an edge only (a non-manifold edge of the hull mesh)."""
    z, y, x = np.meshgrid(*(np.arange(G) + 0.5,) * 3, indexing="ij")
    occ = ((x - 5.2) ** 2 + (y - 5.9) ** 2 + (z - 6.1) ** 2) < 3.6 ** 2
    assert not occ[1:4, 9:12, 9:12].any()
    occ[2, 10, 10] = occ[2, 11, 11] = True
    return occ.astype(np.uint8)[None]


def voxel_centres(occ, origin, voxel):
    """The centres of the lattice's voxels, occupied or not, (G^3, 3) float32 in x, y, z."""
    _, Gz, Gy, Gx = occ.shape
    z, y, x = np.meshgrid(np.arange(Gz) + 0.5, np.arange(Gy) + 0.5, np.arange(Gx) + 0.5, indexing="ij")
    return (np.asarray(origin) + voxel * np.stack([x.ravel(), y.ravel(), z.ravel()], 1)).astype(np.float32)


def soup(seed: int = 5, F: int = 2000, P: int = 4096):
    """F random overlapping triangles (edges about a fifth of the cloud's extent) and P points among them."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, (F, 1, 3))
    verts = (centre + 0.2 * rng.standard_normal((F, 3, 3))).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * F, dtype=np.int64).reshape(F, 3), rng.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)


def clusters(seed: int = 9, F_each: int = 1024, apart: float = 100.0):
    """Two clusters of F_each small faces, each inside a unit cube, the second moved by `apart` along every axis: (verts, faces,
    the first cluster's vertices)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.1, 0.9, (2, F_each, 1, 3))
    tri = centre + 0.05 * rng.uniform(-1, 1, (2, F_each, 3, 3))
    tri[1] += apart
    verts = tri.reshape(-1, 3).astype(np.float32)
    return verts, np.arange(6 * F_each, dtype=np.int64).reshape(-1, 3), verts[:3 * F_each].copy()
