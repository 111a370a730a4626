"""Inputs shared by the CPU and GPU tests of the point <-> mesh distances: hand cases with known answers on the 1/8 grid (exact in
float32 and float64), seeded meshes and clouds, and the batches that walk the edges of the launch."""
import numpy as np

TILE = 128  # PM_TILE of smilify_amd/csrc/point_mesh.hip (tests/test_point_mesh_cpu.py reads the source and compares)
TRI = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]  # a, b, c

# (name, triangle, point, barycentrics of the closest point, squared distance): every coordinate a multiple of 1/8
HAND = [
    # one point in each of the seven regions
    ("A", TRI, [-0.5, -0.25, 0.5], [1, 0, 0], 0.5625),
    ("B", TRI, [1.5, -0.25, 0.0], [0, 1, 0], 0.3125),
    ("C", TRI, [-0.25, 1.5, 0.25], [0, 0, 1], 0.375),
    ("AB", TRI, [0.5, -0.5, 0.25], [0.5, 0.5, 0], 0.3125),
    ("AC", TRI, [-0.5, 0.25, 0.0], [0.75, 0, 0.25], 0.25),
    ("BC", TRI, [1.0, 1.0, 0.0], [0, 0.5, 0.5], 0.5),
    ("interior", TRI, [0.25, 0.25, 0.5], [0.5, 0.25, 0.25], 0.25),
    # on the triangle: exactly 0
    ("on the face", TRI, [0.25, 0.5, 0.0], [0.25, 0.25, 0.5], 0.0),
    ("on an edge", TRI, [0.5, 0.5, 0.0], [0, 0.5, 0.5], 0.0),
    ("on a vertex", TRI, [1.0, 0.0, 0.0], [0, 1, 0], 0.0),
    # on the boundaries between regions: the earlier region of the walk decides, the closest point is the same
    ("A | AB | AC above a", TRI, [0.0, 0.0, 1.0], [1, 0, 0], 1.0),
    ("AB | interior", TRI, [0.5, 0.0, 0.5], [0.5, 0.5, 0], 0.25),
    ("B | AB", TRI, [1.0, -0.5, 0.0], [0, 1, 0], 0.25),
    ("BC | interior", TRI, [0.5, 0.5, 0.25], [0, 0.5, 0.5], 0.0625),
    ("C | AC", TRI, [-0.5, 1.0, 0.0], [0, 0, 1], 0.25),
]

# (name, triangle, point, closest point, squared distance): the three degenerate kinds; the barycentrics of equal vertices are free
DEGENERATE = [
    ("a == b: the segment a c", [[0, 0, 0], [0, 0, 0], [1, 0, 0]], [0.5, 0.5, 0.0], [0.5, 0, 0], 0.25),
    ("a == b: before a", [[0, 0, 0], [0, 0, 0], [1, 0, 0]], [-1.0, 0.0, 0.0], [0, 0, 0], 1.0),
    ("a == b: beyond c", [[0, 0, 0], [0, 0, 0], [1, 0, 0]], [2.0, 1.0, 0.0], [1, 0, 0], 2.0),
    ("a == c: the segment a b", [[0, 0, 0], [1, 0, 0], [0, 0, 0]], [0.25, 0.0, 0.5], [0.25, 0, 0], 0.25),
    ("b == c: the segment a b", [[0, 0, 0], [1, 0, 0], [1, 0, 0]], [0.75, -0.5, 0.0], [0.75, 0, 0], 0.25),
    ("collinear a b c: inside b c", [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [1.5, 0.5, 0.0], [1.5, 0, 0], 0.25),
    ("collinear a b c: beyond c", [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [3.0, 0.0, 1.0], [2, 0, 0], 2.0),
    ("collinear a b c: before a", [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [-1.0, 1.0, 0.0], [0, 0, 0], 2.0),
    ("collinear b a c: a in the middle", [[0, 0, 0], [-1, 0, 0], [1, 0, 0]], [0.5, 0.0, 0.5], [0.5, 0, 0], 0.25),
    ("collinear b a c: beyond b", [[0, 0, 0], [-1, 0, 0], [1, 0, 0]], [-5.0, 0.0, 0.0], [-1, 0, 0], 16.0),
    ("a == b == c: a point", [[0.5, 0.5, 0.5]] * 3, [1.0, 0.5, 0.5], [0.5, 0.5, 0.5], 0.25),
]


def hand_mesh(cases):
    """The triangles of `cases` as one mesh with three vertices per face: (verts (3K,3) float32, faces (K,3), points (K,3) float32);
    point r is meant for face r only (the tests evaluate pairs, or give every case a mesh of its own)."""
    verts = np.asarray([c[1] for c in cases], np.float32).reshape(-1, 3)
    faces = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
    return verts, faces, np.asarray([c[2] for c in cases], np.float32)


def tie_fan(n_faces: int = 389, apex_faces=(130, 131, 260, 388)):
    """A mesh in which the faces `apex_faces` share the vertex (0,0,0), which is the closest point of each of them to (0,0,1) at the
    squared distance 1 exactly, while every other face is far away: (verts, faces, point, the face that must win = the smallest)."""
    ring = np.asarray([[1, 0, -1], [0, 1, -1], [-1, 0, -1], [0, -1, -1]], np.float32)
    verts = [np.zeros(3, np.float32)] + list(ring)
    faces = []
    rng = np.random.default_rng(3)
    for j in range(n_faces):
        if j in apex_faces:
            k = apex_faces.index(j) % 4
            faces.append([0, 1 + k, 1 + (k + 1) % 4])
        else:
            base = len(verts)
            verts += list((8.0 + rng.integers(0, 16, (3, 3)) / 8.0).astype(np.float32))
            faces.append([base, base + 1, base + 2])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64), np.asarray([[0.0, 0.0, 1.0]], np.float32), min(apex_faces)


def random_mesh(seed: int, V: int, F: int, scale: float = 1.0, degenerate: bool = False):
    """A seeded soup of F faces over V float32 vertices (not a surface: every region and every relative position occurs).  With
    `degenerate` every eighth face repeats a vertex, every eighth (offset 1) is collinear and every eighth (offset 2) is a point."""
    rng = np.random.default_rng(seed)
    verts = (rng.standard_normal((V, 3)) * scale).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int64)
    if degenerate:
        verts = np.concatenate([verts, np.zeros((F, 3), np.float32)])
        for j in range(F):
            if j % 8 == 0:
                faces[j, 1] = faces[j, 0]
            elif j % 8 == 1:  # the third vertex exactly half way between the other two, on the 1/8 grid
                a, b = np.round(verts[faces[j, 0]] * 4) / 4, np.round(verts[faces[j, 1]] * 4) / 4
                verts[faces[j, 0]], verts[faces[j, 1]], verts[V + j] = a, b, (a + b) / 2
                faces[j, 2] = V + j
            elif j % 8 == 2:
                faces[j] = faces[j, 0]
    return verts, faces


def random_cloud(seed: int, P: int, scale: float = 1.5):
    return (np.random.default_rng(seed).standard_normal((P, 3)) * scale).astype(np.float32)


def launch_sizes(tile: int = TILE):
    """(F, P) pairs at the edges of the launch: faces around one tile and in several, points around one wave and in several blocks."""
    return [(F, P) for F in (1, tile - 1, tile, tile + 1, 3 * tile + 5) for P in (1, 63, 64, 65, 257)]


def batch(tile: int = TILE, seed: int = 11):
    """N = 3 meshes of different sizes with clouds padded to P = 257 and lengths (257, 0, 65): [(verts, faces)], points (3,257,3),
    lengths (3,)."""
    sizes = [(40, 3 * tile + 5), (7, tile - 1), (90, tile + 1)]
    meshes = [random_mesh(seed + n, V, F, scale=2.0 ** -n) for n, (V, F) in enumerate(sizes)]
    points = np.stack([random_cloud(seed + 10 + n, 257, 2.0 ** -n) for n in range(3)])
    return meshes, points, np.asarray([257, 0, 65], np.int32)
