"""GPU tests of the mesh hierarchy (``pytest -m gpu``): ``mesh3d.MeshBVH`` and the ``bvh=`` keyword against the brute force of
csrc/point_mesh.hip on the same inputs.  The hierarchy promises the brute force's winner, so every comparison is ``torch.equal`` on
dist2, face and bary: there is no tolerance anywhere in this file.  Every case runs with the queries in the caller's order and in
Morton order."""
import functools

import numpy as np
import pytest
import torch

import mesh_bvh_cases as BC
import point_mesh_cases as PC
import winding_cases as WC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _meshes(*vf):
    from smilify_amd.mesh3d import Meshes

    return Meshes([torch.as_tensor(np.asarray(v), dtype=torch.float32).reshape(-1, 3).to(DEV) for v, _ in vf],
                  [torch.as_tensor(np.asarray(f)).long().reshape(-1, 3).to(DEV) for _, f in vf])


def _pts(p):
    p = torch.as_tensor(np.asarray(p) if not isinstance(p, torch.Tensor) else p, dtype=torch.float32).to(DEV)
    return p[None] if p.dim() == 2 else p


def _same(meshes, points, lengths=None, name="", bvh=None):
    """The hierarchy's answers equal the brute force's, bit for bit, sorted queries or not; returns the brute force's."""
    from smilify_amd import mesh3d

    points = _pts(points)
    want = mesh3d.closest_points(meshes, points, lengths)
    for sort_queries in (False, True):
        tree = mesh3d.MeshBVH(meshes, sort_queries=sort_queries) if bvh is None else bvh
        tree.sort_queries = sort_queries
        for got in (tree.closest_points(points, lengths), mesh3d.closest_points(meshes, points, lengths, bvh=tree)):
            for field in ("dist2", "face", "bary", "points"):
                a, b = getattr(got, field), getattr(want, field)
                assert a.dtype == b.dtype and torch.equal(a, b), (name, sort_queries, field, int((a != b).sum()))
    return want


# ---- 1: the existing generators -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cases", ["HAND", "DEGENERATE"])
def test_hand_cases(cases):
    verts, faces, points = PC.hand_mesh(getattr(PC, cases))
    got = _same(_meshes((verts, faces)), points, name=cases)
    assert (got.face >= 0).all()
    for r in range(len(points)):  # and every case as a mesh of its own
        _same(_meshes((verts[3 * r:3 * r + 3], [[0, 1, 2]])), points[r:r + 1], name=f"{cases}[{r}]")


def test_tie_fan():
    verts, faces, point, winner = PC.tie_fan()
    got = _same(_meshes((verts, faces)), point, name="tie fan")
    assert int(got.face[0, 0]) == winner and float(got.dist2[0, 0]) == 1.0


@pytest.mark.parametrize("degenerate", [False, True])
def test_random_meshes(degenerate):
    verts, faces = PC.random_mesh(21, 70, 3 * PC.TILE + 5, degenerate=degenerate)
    _same(_meshes((verts, faces)), PC.random_cloud(22, 513), name=f"random degenerate={degenerate}")


def test_batch_with_lengths():
    meshes, points, lengths = PC.batch()
    got = _same(_meshes(*meshes), points, torch.from_numpy(lengths).to(DEV), name="batch")
    assert (got.face[1] == -1).all() and (got.face[2, 65:] == -1).all() and (got.face[0] >= 0).all()


def test_launch_sizes():
    for F, P in PC.launch_sizes():
        verts, faces = PC.random_mesh(100 + F, 50, F)
        _same(_meshes((verts, faces)), PC.random_cloud(200 + P, P), name=f"F={F} P={P}")


# ---- 2: where a tree can go wrong -----------------------------------------------------------------------------------------------
def test_face_and_point_counts():
    from smilify_amd import mesh3d

    for F in BC.face_counts():
        verts, faces = PC.random_mesh(300 + F, 40, F)
        meshes = _meshes((verts, faces))
        if F == 0:  # one mesh without a face: refused by the brute force and by the hierarchy alike
            with pytest.raises(ValueError):
                mesh3d.closest_points(meshes, _pts(PC.random_cloud(1, 4)))
            with pytest.raises(ValueError):
                mesh3d.MeshBVH(meshes)
            continue
        for P in BC.POINT_COUNTS:
            _same(meshes, PC.random_cloud(400 + P, P), name=f"F={F} P={P}")


def test_batch_with_an_empty_mesh():
    sizes = [(30, 129), (5, 0), (60, 1000)]
    meshes = _meshes(*[PC.random_mesh(500 + n, V, F) for n, (V, F) in enumerate(sizes)])
    points = np.stack([PC.random_cloud(510 + n, 257) for n in range(3)])
    got = _same(meshes, points, name="empty mesh in a batch")
    assert (got.face[1] == -1).all() and torch.isinf(got.dist2[1]).all() and (got.face[0] >= 0).all() and (got.face[2] >= 0).all()


def test_copies_of_one_triangle():
    verts, faces = BC.copies(300)
    got = _same(_meshes((verts, faces)), PC.random_cloud(31, 257, 1.0), name="copies")
    assert (got.face == 0).all()


def test_lattice_ties():
    verts, faces, points = BC.lattice(32)
    got = _same(_meshes((verts, faces)), points, name="lattice")
    assert (got.dist2 == 0).all()


def test_hull_mesh_at_its_voxel_centres():
    from smilify_amd import engine
    from smilify_amd import visual_hull as VH
    from smilify_amd.mesh3d import Meshes

    occ = BC.hull_occupancy()
    G = occ.shape[-1]
    hull = VH.VisualHull(torch.from_numpy(occ).to(DEV), None, None, engine.HullGridSpec(1, (G, G, G), WC.HULL_ORIGIN, WC.HULL_VOXEL))
    for steps in ((), VH.taubin_steps(2)):
        mesh = hull.extract_mesh(relax_steps=steps, return_normals=False)
        meshes = Meshes([mesh.verts.float()], [mesh.faces.long()])
        got = _same(meshes, BC.voxel_centres(occ, WC.HULL_ORIGIN, WC.HULL_VOXEL), name=f"hull {len(steps)}")
        assert (got.face >= 0).all()


def test_soup():
    verts, faces, points = BC.soup()
    _same(_meshes((verts, faces)), points, name="soup")


@functools.lru_cache(maxsize=1)
def _atta_clouds():
    verts, faces = WC.atta()
    on, normal = WC._on_faces(np.random.default_rng(41), verts, faces, 1024)
    extent = float(np.abs(verts).max())
    clouds = [verts, on.astype(np.float32)]
    for k in (-14, -18, -22):
        for sign in (1.0, -1.0):
            clouds.append((on + sign * extent * 2.0 ** k * normal).astype(np.float32))
    return verts, faces, clouds


def test_atta_scan():
    verts, faces, clouds = _atta_clouds()
    meshes = _meshes((verts, faces))
    for i, cloud in enumerate(clouds):
        _same(meshes, cloud, name=f"atta cloud {i}")


def test_far_points_and_scaling():
    from smilify_amd import mesh3d

    verts, faces, clouds = _atta_clouds()
    rng = np.random.default_rng(43)
    far = (100.0 * rng.standard_normal((257, 3))).astype(np.float32)
    _same(_meshes((verts, faces)), far, name="far points")
    near = np.concatenate([clouds[2][:400], PC.random_cloud(44, 113, 0.7)])
    base = _same(_meshes((verts, faces)), near, name="scale 1")
    for k in (20, -20):
        s = np.float32(2.0 ** k)
        got = _same(_meshes((verts * s, faces)), near * s, name=f"scale 2^{k}")
        tree = mesh3d.MeshBVH(_meshes((verts * s, faces))).closest_points(_pts(near * s))
        assert torch.equal(tree.face, base.face) and torch.equal(got.face, base.face)
        assert torch.equal(tree.dist2, base.dist2 * float(s) ** 2) and torch.equal(tree.bary, base.bary)


def test_invalid_points_and_faces():
    verts, faces = PC.random_mesh(51, 60, 300)
    verts, faces = verts.copy(), faces.copy()
    verts[7] = np.nan  # every face of vertex 7 is unusable
    verts[9, 1] = np.inf
    faces[5] = [0, 1, 60]  # out of range
    faces[11] = [-1, 2, 3]
    points = PC.random_cloud(52, 300)
    points[3] = np.nan
    points[40, 2] = np.inf
    points[41, 0] = -np.inf
    points[77] = 3.2e38
    meshes = _meshes((verts, faces))
    got = _same(meshes, points, name="invalid")
    bad = torch.tensor([3, 40, 41, 77], device=DEV)
    assert (got.face[0, bad] == -1).all() and torch.isinf(got.dist2[0, bad]).all() and (got.bary[0, bad] == 0).all()
    unusable = set(np.nonzero((faces == 7).any(1) | (faces == 9).any(1))[0].tolist()) | {5, 11}
    assert not (set(got.face[0].tolist()) & unusable) and int((got.face[0] >= 0).sum()) == 296
    # a mesh of unusable faces only: nothing wins.  Compared on the kernels' own outputs: closest_points() would look up the vertices
    # of face 0 for its fourth field, and that face's indices lie outside the vertex array here.
    from smilify_amd import engine, mesh3d

    none = _meshes((verts, faces[[5, 11, 5]]))
    mt, v, p = none.face_tables(), none.verts_packed().contiguous(), _pts(points[:9])
    want = engine.point_mesh_distance(v, mt, p)
    for sort_queries in (False, True):
        got = mesh3d.MeshBVH(none, sort_queries=sort_queries).query(p, want_evaluated=True)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], want)) and (got[1] == -1).all() and torch.isinf(got[0]).all()
        assert got[3].tolist() == [[3, 3, 3, 0, 3, 3, 3, 3, 3]]  # (the NaN point evaluates nothing)


# ---- 3, 4: the build's invariants, two builds, refit ---------------------------------------------------------------------------------
def _check_tree(meshes, tree, name):
    """order is a permutation per mesh; every leaf box is the float32 min / max of its usable faces' vertices; every inner box the union
    of its children."""
    arr = tree.arrays()
    order, boxes, leaf = arr["order"].cpu().numpy(), arr["boxes"].cpu().numpy(), arr["leaf_size"]
    assert leaf == BC.leaf_size()
    f0 = 0
    for n, (v, f) in enumerate(zip(meshes.verts_list(), meshes.faces_list())):
        v, f = v.cpu().numpy(), f.cpu().numpy()
        F, L, Lp, node0 = len(f), arr["leaves"][n], arr["padded_leaves"][n], arr["node0"][n]
        mine = order[f0:f0 + F]
        assert sorted(mine.tolist()) == list(range(F)), name
        assert L == -(-F // leaf) and Lp >= max(L, 1) and Lp & (Lp - 1) == 0 and (Lp < 2 * L or L <= 1), name
        inside = ((f >= 0) & (f < len(v))).all(1)
        tri = v[np.clip(f, 0, len(v) - 1)]
        usable = inside & np.isfinite(tri).all((1, 2))
        heap = boxes[node0:node0 + 2 * Lp]
        for k in range(Lp):
            ids = [j for j in mine[k * leaf:(k + 1) * leaf] if usable[j]]
            want = np.concatenate([tri[ids].min((0, 1)), tri[ids].max((0, 1))]) if ids else np.asarray([np.inf] * 3 + [-np.inf] * 3, np.float32)
            assert np.array_equal(heap[Lp + k], want), (name, n, k)
        for i in range(1, Lp):
            want = np.concatenate([np.minimum(heap[2 * i, :3], heap[2 * i + 1, :3]), np.maximum(heap[2 * i, 3:], heap[2 * i + 1, 3:])])
            assert np.array_equal(heap[i], want), (name, n, i)
        f0 += F


def test_build_invariants_and_two_builds():
    from smilify_amd import mesh3d

    verts, faces = PC.random_mesh(61, 80, 1000, degenerate=True)
    verts = verts.copy()
    verts[3] = np.nan
    batch = [(verts, faces), PC.random_mesh(62, 5, 0), PC.random_mesh(63, 30, BC.leaf_size() + 1), PC.random_mesh(64, 30, 129)]
    meshes = _meshes(*batch)
    a, b = mesh3d.MeshBVH(meshes), mesh3d.MeshBVH(meshes)
    _check_tree(meshes, a, "build")
    for key in ("order", "boxes"):
        x, y = a.arrays()[key], b.arrays()[key]
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), key  # (bits; the rows no node owns are zero)
    # unusable faces stand behind the usable ones of their mesh
    order = a.arrays()["order"][:1000].cpu().numpy()
    bad = (faces == 3).any(1)[order]
    assert bad.any() and not bad[:int((~bad).sum())].any()


def test_refit_after_large_displacements():
    from smilify_amd import mesh3d

    verts, faces, points = BC.soup(7, 1500, 1024)
    meshes = _meshes((verts, faces), PC.random_mesh(71, 40, 200))
    points = np.stack([points, PC.random_cloud(72, 1024)])
    tree = mesh3d.MeshBVH(meshes)
    before = tree.arrays()["order"].clone()
    extent = float(np.abs(verts).max())
    rng = np.random.default_rng(73)
    moved = meshes.offset_verts(torch.from_numpy((0.1 * extent * rng.standard_normal((len(verts) + 40, 3))).astype(np.float32)).to(DEV))
    assert tree.refit(moved) is tree and torch.equal(tree.arrays()["order"], before)
    _check_tree(moved, tree, "refit")
    _same(moved, points, name="refit", bvh=tree)
    fresh = mesh3d.MeshBVH(moved)
    assert torch.equal(fresh.closest_points(_pts(points)).face, tree.closest_points(_pts(points)).face)
    with pytest.raises(ValueError):
        tree.refit(_meshes((verts, faces)))


# ---- 5: it prunes ----------------------------------------------------------------------------------------------------------------
def test_it_prunes():
    """Two clusters 100 of their sizes apart, queried at the first one's vertices: nearest first reaches the query's own cluster, best
    is 0 there at the latest when the vertex's face is met, and no box of the other cluster alone can be entered again; so at most the
    first cluster and the leaves that mix the two are evaluated."""
    from smilify_amd import mesh3d

    verts, faces, points = BC.clusters()
    F = len(faces)
    meshes = _meshes((verts, faces))
    assert BC.leaf_size() <= F // 4
    for sort_queries in (False, True):
        tree = mesh3d.MeshBVH(meshes, sort_queries=sort_queries)
        count = tree.evaluated(_pts(points))
        print(f"\n[mesh-bvh] prune sort_queries={sort_queries}: evaluated faces per point mean {float(count.float().mean()):.1f} "
              f"max {int(count.max())} of F={F}")
        assert count.dtype == torch.int32 and int(count.min()) >= 1 and int(count.max()) <= 3 * F // 4
    _same(meshes, points, name="clusters")


# ---- 6: autograd -----------------------------------------------------------------------------------------------------------------
def test_autograd_equal_bits():
    from smilify_amd import fit3d, mesh3d

    verts, faces, clouds = _atta_clouds()
    meshes0 = _meshes((verts, faces))
    tree = mesh3d.MeshBVH(meshes0)
    pts0 = _pts(np.concatenate([clouds[2][:300], PC.random_cloud(81, 213, 0.8)]))
    out = []
    for bvh in (None, tree):
        offs = torch.zeros(len(verts), 3, device=DEV, requires_grad=True)
        pts = pts0.clone().requires_grad_(True)
        meshes = meshes0.offset_verts(offs)
        dist2, face = fit3d.point_face_distance(meshes, pts, bvh=bvh)
        w = torch.linspace(0.5, 1.5, dist2.numel(), device=DEV).view_as(dist2)
        (w * dist2).sum().backward()
        out.append((dist2.detach(), face, pts.grad, offs.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[0][3].abs().max()) > 0
    # the one-sided losses and the signed distance
    ball_v, ball_f = WC.icosphere(2)
    ball = _meshes((ball_v, ball_f))
    tree = mesh3d.MeshBVH(ball)
    cloud = _pts(PC.random_cloud(82, 400, 0.8))
    for fn in (fit3d.containment_loss, fit3d.penetration_loss):
        got = []
        for bvh in (None, tree):
            p = cloud.clone().requires_grad_(True)
            loss = fn(ball, p, bvh=bvh)
            loss.backward()
            got.append((loss.detach(), p.grad))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and float(got[0][0]) > 0
    a, b = fit3d.point_mesh_signed_distance(ball, cloud), fit3d.point_mesh_signed_distance(ball, cloud, bvh=tree)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[0] < 0).any() and (a[0] > 0).any()
    s, t = mesh3d.signed_distance(ball, cloud), mesh3d.signed_distance(ball, cloud, bvh=tree)
    assert all(torch.equal(x, y) for x, y in zip(s, t))


# ---- 8: the C ABI's edges --------------------------------------------------------------------------------------------------------
def test_abi_edges():
    from smilify_amd import _lib, engine

    lib = _lib.load()
    assert lib.smil_bvh_workspace_bytes(0, 10, 4, 9) == 0 and lib.smil_bvh_workspace_bytes(1, 0, 4, 9) == 0
    assert lib.smil_bvh_workspace_bytes(1, 10, 0, 9) == 0 and lib.smil_bvh_workspace_bytes(65536, 10, 4, 9) == 0
    assert lib.smil_bvh_nodes(0, 10) == 0 and lib.smil_bvh_nodes(1, 0) == 0
    small, large = lib.smil_bvh_workspace_bytes(2, 100, 50, 60), lib.smil_bvh_workspace_bytes(2, 1000, 500, 600)
    assert 0 < small < large and small % 256 == 0 and small > lib.smil_point_mesh_workspace_bytes(2, 100, 50, 60)
    assert lib.smil_bvh_nodes(3, 1000) == 4 * (1000 // BC.leaf_size() + 3)
    verts, faces = PC.random_mesh(91, 30, 50)
    meshes = _meshes((verts, faces))
    mt, v = meshes.face_tables(), meshes.verts_packed().contiguous()
    order, boxes = engine.bvh_build(v, mt)
    pts = _pts(PC.random_cloud(92, 33))
    ws = torch.empty(int(lib.smil_bvh_workspace_bytes(1, 50, 33, 30)), dtype=torch.uint8, device=DEV)
    d2, face, bary = torch.empty(1, 33, device=DEV), torch.empty(1, 33, dtype=torch.int32, device=DEV), torch.empty(1, 33, 3, device=DEV)
    P = engine._ptr

    def call(N=1, F=50, max_faces=50, n_pts=33, order_=order, d2_=d2):
        return lib.smil_bvh_point_face_distance(P(v), 30, P(mt.faces), P(mt.face_off), N, F, max_faces, P(order_), P(boxes), P(pts), n_pts, None,
                                                P(d2_), P(face), P(bary), None, P(ws), None)

    assert call() == 0  # NULL for the count, NULL lengths
    torch.cuda.synchronize()
    want = engine.point_mesh_distance(v, mt, pts)
    assert torch.equal(d2, want[0]) and torch.equal(face, want[1]) and torch.equal(bary, want[2])
    for bad in (dict(N=0), dict(F=0), dict(n_pts=0), dict(max_faces=0), dict(max_faces=51), dict(order_=None), dict(d2_=None)):
        assert call(**bad) == _lib.E_INVALID, bad
        assert b"smil_bvh_point_face_distance" in lib.smil_last_error()
    keys = torch.empty(50, dtype=torch.int64, device=DEV)
    assert lib.smil_bvh_codes(P(v), 30, P(mt.faces), P(mt.face_off), 1, 0, 50, P(keys), P(ws), None) == _lib.E_INVALID
    assert lib.smil_bvh_build(P(v), 30, P(mt.faces), P(mt.face_off), 1, 50, 50, None, P(order), P(boxes), P(ws), None) == _lib.E_INVALID
    assert lib.smil_bvh_refit(P(v), 0, P(mt.faces), P(mt.face_off), 1, 50, 50, P(order), P(boxes), P(ws), None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        engine.bvh_point_face_distance(v, mt, order[:-1], boxes, pts)
