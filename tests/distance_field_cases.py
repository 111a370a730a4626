"""TEST INFRASTRUCTURE ONLY: seeded occupancy patterns and sample points for the distance-field tests.

``patterns(G)`` is a stack of frames of grid ``G = (Gx, Gy, Gz)``: a single voxel in each of the 8 corners, two opposite corners, a plane, a
checkerboard, random at density 0.5 and 0.01, a full frame, and an all-empty frame between two full ones (frames must not leak into each
other).  ``reference(G, invert, border)`` is ``edt_brute`` of it, computed once and shared: leave it unchanged.

The kernel's paths (csrc/distance_field.hip): a z-slice of up to 4 096, 16 384 or 65 536 cells takes x and y fused in LDS (three
instantiations), a larger one the x pass in global memory and a line pass for y; a y or z line of up to 32, 128, 256 or ``LDS_LINE`` = 512 cells is
searched in LDS, a longer one in global memory.  ``SHAPES`` are the small extents at which a line kernel can go wrong, ``PATH_SHAPES`` one
grid per remaining path, with sparse patterns (``sparse_patterns``) so that the pairs stay few.
"""
import functools

import numpy as np

import distance_field_ref as DR

LDS_LINE = 512     # EDT_MAX_LINE: the longest y or z line the LDS path holds
LDS_SLICE = 65536  # EDT_MAX_SLICE: the largest z-slice the fused x-y kernel holds
SHAPES = [(gx, gy, gz) for gx in (1, 2, 63, 64, 65, 130) for gy in (1, 3, 5) for gz in (1, 3, 5)] + [(3, 65, 2), (2, 3, 130)]
PATH_SHAPES = [
    (130, 33, 2),            # a slice of 4 290 cells: the second fused instantiation
    (129, 128, 1),           # 16 512 cells: the third (1 024 threads)
    (3, 2, 33), (2, 3, 129), (2, 3, 257),  # z lines of the second, third and fourth LDS instantiation
    (2, 3, LDS_LINE + 1),    # a z line one beyond the LDS path: searched in global memory, from one buffer into another
    (257, 256, 2),           # a slice of 65 792 cells: x pass in global memory, y (256) and z through the LDS line kernel
    (128, LDS_LINE + 1, 1),  # 65 664 cells and a y line one beyond the LDS path; no z pass: the result is copied back
]
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (invert, border)
NAMES = [f"corner{c}" for c in range(8)] + ["opposite", "plane", "checker", "random50", "random01", "full", "full_a", "empty", "full_b"]


def patterns(G, seed=0):
    """(17,Gz,Gy,Gx) uint8 (values 0, 1 and - in the random frames - 255: any non-zero byte is occupied)."""
    Gx, Gy, Gz = G
    rng = np.random.default_rng(seed + Gx + 131 * Gy + 1031 * Gz)
    occ = np.zeros((len(NAMES), Gz, Gy, Gx), np.uint8)
    for c in range(8):
        occ[c, (Gz - 1) * (c >> 2 & 1), (Gy - 1) * (c >> 1 & 1), (Gx - 1) * (c & 1)] = 1
    occ[8, 0, 0, 0] = occ[8, Gz - 1, Gy - 1, Gx - 1] = 1
    occ[9, :, :, Gx // 2] = 1  # the plane i = Gx / 2
    k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    occ[10] = (i + j + k) % 2
    occ[11] = (rng.random((Gz, Gy, Gx)) < 0.5) * 255
    occ[12] = (rng.random((Gz, Gy, Gx)) < 0.01) * 255
    occ[13] = occ[14] = occ[16] = 1
    return occ


def sparse_patterns(G, seed=0):
    """(3,Gz,Gy,Gx) uint8: features at density 0.003, an empty frame, features at density 0.003 - and the complement of all that, so that
    ``invert`` sees the same few features: ``[plain, inverted]``."""
    Gx, Gy, Gz = G
    rng = np.random.default_rng(seed + Gx + 131 * Gy + 1031 * Gz)
    occ = (rng.random((3, Gz, Gy, Gx)) < 0.003).astype(np.uint8)
    occ[1] = 0
    occ[0, 0, 0, 0] = occ[2, Gz - 1, Gy - 1, Gx - 1] = 1
    return [occ, (1 - occ).astype(np.uint8)]


@functools.lru_cache(maxsize=None)
def reference(G, invert, border):
    return DR.edt_brute(patterns(G), invert, border)


@functools.lru_cache(maxsize=None)
def sparse_reference(G, invert, border):
    """``shell_pairs=False``: the shells of these grids hold up to 135 000 voxels."""
    return DR.edt_brute(sparse_patterns(G)[invert], invert, border, shell_pairs=False)


def blob(G, N=3, seed=0):
    """(N,Gz,Gy,Gx) uint8: a seeded ellipsoid per frame, well inside the grid where the grid has room - a hull-like occupancy for the
    sampler's tests (signed fields need an inside)."""
    Gx, Gy, Gz = G
    rng = np.random.default_rng(seed + 17)
    k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    occ = np.zeros((N, Gz, Gy, Gx), np.uint8)
    for n in range(N):
        c = (np.array([Gx, Gy, Gz]) - 1) * rng.uniform(0.35, 0.65, 3)
        r = np.maximum(np.array([Gx, Gy, Gz]) * rng.uniform(0.2, 0.35, 3), 0.8)
        occ[n] = ((i - c[0]) / r[0]) ** 2 + ((j - c[1]) / r[1]) ** 2 + ((k - c[2]) / r[2]) ** 2 <= 1.0
    return occ


def sample_points(G, origin, voxel, N, P, dim, seed=0):
    """(N,P,dim) float32 covering, in this order and then repeating with fresh random draws: cell centres (exact when origin and voxel
    are dyadic), random positions inside the grid, outside it beyond one face, beyond an edge and beyond a corner (both sides), NaN and
    infinite coordinates.  Row P - 1 of frame 0 is always a NaN point when P > 1."""
    Gx, Gy, Gz = G
    ext = np.array([Gx, Gy, Gz], np.float64)[:dim]
    rng = np.random.default_rng(seed + 7 * P + dim)
    origin = np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 3), (N, 3))[:, :dim]
    voxel = np.broadcast_to(np.asarray(voxel, np.float64).reshape(-1), (N,))
    u = np.empty((N, P, len(ext)))  # the continuous index + 0.5 (0 .. G across the grid), (x, y[, z])
    for p in range(P):
        kind = p % 8
        if kind == 0:    # a cell centre
            u[:, p] = np.floor(rng.uniform(0, 1, (N, len(ext))) * ext) + 0.5
        elif kind in (1, 2):
            u[:, p] = rng.uniform(0.5, np.maximum(ext - 0.5, 0.5), (N, len(ext)))
        else:            # outside on 1, 2 or all axes, on either side
            u[:, p] = rng.uniform(0.5, np.maximum(ext - 0.5, 0.5), (N, len(ext)))
            axes = rng.permutation(len(ext))[: min(kind - 2, len(ext))] if kind < 6 else np.arange(len(ext))
            for a in axes:
                side = rng.integers(0, 2, N)
                u[:, p, a] = np.where(side == 1, ext[a] + rng.uniform(0.0, 3.0, N), -rng.uniform(0.0, 3.0, N))
    pts = (origin[:, None, :] + u * voxel[:, None, None]).astype(np.float32)
    if P > 1:
        pts[0, P - 1, 0] = np.nan
    if P > 8:
        pts[N - 1, P - 2, len(ext) - 1] = np.inf
        pts[N - 1, P - 3, 0] = -np.inf
    return pts[..., ::-1].copy() if dim == 2 else pts
