"""CPU checks of the 3-D registration plumbing: OBJ loading, the fixture, the regulariser topology tables against brute force,
known answers of the float64 oracle, and argument validation of the new C entry points (no GPU touched)."""
import ctypes
import os

import numpy as np
import torch

import mesh3d_ref as ref
from conftest import GOLDEN


def test_load_obj_quads_negative_and_slash_indices(tmp_path):
    from smilify_amd.mesh3d import load_obj

    p = tmp_path / "m.obj"
    p.write_text("# comment\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
                 "f 1/1 2/1 3/1 4/1\n"      # quad, i/j
                 "f -4//1 -3//1 -1//1\n"    # negative, i//k
                 "f 2/1/1 3/1/1 4/1/1\n"    # i/j/k
                 "v 0 0 1\nf 1 2 5 3 4\n"  # pentagon after one more vertex; plain indices
                 "o name\nusemtl x\n")
    v, f = load_obj(str(p))
    assert v.shape == (5, 3) and v.dtype == torch.float32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3], [0, 1, 4], [0, 4, 2], [0, 2, 3]]


def test_load_obj_rejects_bad_index(tmp_path):
    from smilify_amd.mesh3d import load_obj

    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    try:
        load_obj(str(p))
    except ValueError as e:
        assert "out of range" in str(e)
    else:
        raise AssertionError("an out-of-range face index was accepted")


def test_atta_fixture_counts():
    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    assert d["verts"].shape == (5246, 3) and d["faces"].shape == (10878, 3)
    assert d["faces"].min() >= 0 and d["faces"].max() < 5246


def test_topology_against_brute_force(tables):
    from smilify_amd.mesh3d import Topology

    expect = {"stick": (9047, 9012), "mouse": (28538, 23722)}
    for key in ("stick", "mouse", "synthetic"):
        t = tables(key)
        T = Topology(t.faces, t.V)
        e = ref.edges_brute(t.faces)
        p = ref.normal_pairs_brute(t.faces)
        assert np.array_equal(T.edges, e), key
        canon = lambda a: sorted(map(tuple, np.concatenate([a[:, :2], np.sort(a[:, 2:], axis=1)], axis=1).tolist()))  # noqa: E731
        assert canon(T.pairs) == canon(p), key
        if key in expect:
            assert (T.E, T.Q) == expect[key], (key, T.E, T.Q)
        # neighbour CSR: both directions of every edge, 1/deg
        deg = np.bincount(e.reshape(-1), minlength=t.V)
        assert np.array_equal(np.diff(T.nbr_ptr), deg)
        for i in (0, t.V // 2, t.V - 1):
            nb = T.nbr[T.nbr_ptr[i]:T.nbr_ptr[i + 1]]
            assert sorted(nb.tolist()) == sorted(set(e[e[:, 0] == i, 1].tolist()) | set(e[e[:, 1] == i, 0].tolist()))
        assert np.allclose(T.inv_deg[deg > 0], 1.0 / deg[deg > 0])
        # vertex -> pair incidence: every (pair, role) exactly once, under the vertex it names
        codes = T.vpair
        assert sorted(codes.tolist()) == list(range(4 * T.Q))
        owner = np.repeat(np.arange(t.V), np.diff(T.vpair_ptr))
        assert np.array_equal(T.pairs.reshape(-1)[codes], owner)


def test_stick_boundary_and_triple_edges(tables):
    from smilify_amd.mesh3d import Topology

    for key, boundary, triple in (("stick", 39, 2), ("mouse", 4816, 0)):
        t = tables(key)
        T = Topology(t.faces, t.V)
        fe = np.sort(np.concatenate([t.faces[:, [0, 1]], t.faces[:, [1, 2]], t.faces[:, [2, 0]]]), axis=1)
        _, cnt = np.unique(fe, axis=0, return_counts=True)
        assert (cnt == 1).sum() == boundary and (cnt == 3).sum() == triple
        assert T.Q == int((cnt * (cnt - 1) // 2).sum())


def _grid(n=5, z=None):
    xs, ys = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(n * n) if z is None else z], 1)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            f += [[a, b, c], [a, c, d]]
    return torch.from_numpy(v)[None], np.array(f)


def test_oracle_known_answers():
    v, f = _grid()
    assert abs(ref.normal_loss(v, f)) < 1e-12  # a flat grid: every face pair is coplanar and consistently oriented
    n = 5
    V = v.shape[1]
    # interior Laplacian rows of a regular grid are 0 (triangulated grid: each interior vertex's 6 neighbours are symmetric)
    e = ref.edges_brute(f)
    L = np.zeros((V, V))
    deg = np.bincount(e.reshape(-1), minlength=V)
    for a, b in e:
        L[a, b] = 1 / deg[a]
        L[b, a] = 1 / deg[b]
    r = (L - np.eye(V)) @ v[0].numpy()
    interior = [i * n + j for i in range(1, n - 1) for j in range(1, n - 1)]
    assert np.abs(r[interior]).max() < 1e-12
    assert abs(ref.laplacian_loss(v, f) - ref.laplacian_loss_sparse(v, f)) < 1e-12
    # tetrahedron with unit edges along the axes: 3 edges of length 1, 3 of length sqrt(2): mean square = 1.5
    tv = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float64)
    tf = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    assert abs(float(ref.edge_loss(tv, tf)) - 1.5) < 1e-12
    # identical point sets: chamfer 0
    x = torch.randn(2, 50, 3, dtype=torch.float64)
    loss, ix, iy = ref.chamfer(x, x)
    assert float(loss) == 0.0 and torch.equal(ix[0], torch.arange(50))


def test_abi_rejects_bad_arguments():
    from smilify_amd import _lib

    lib = _lib.load()
    dummy = ctypes.c_void_p(16)
    assert lib.smil_chamfer(None, None, 1, 1, 1, 0, 0, 0, None, None, None, None, None, None, None) == -1
    assert b"null argument" in lib.smil_last_error()
    assert lib.smil_chamfer(dummy, dummy, 0, 5, 5, 0, 0, 0, dummy, None, None, None, None, dummy, None) == -1
    assert b"bad sizes" in lib.smil_last_error()
    assert lib.smil_chamfer(dummy, dummy, 1, 5, 5, 0, 0, 0, dummy, None, None, dummy, None, dummy, None) == -1
    assert b"together" in lib.smil_last_error()
    assert lib.smil_chamfer_workspace_bytes(0, 5, 5) == 0
    assert lib.smil_sample_points(None, 3, None, None, None, 1, 10, 0, None, None, None) == -1
    assert lib.smil_sample_points(dummy, 3, dummy, dummy, dummy, 0, 10, 0, dummy, None, None) == -1
    assert b"bad sizes" in lib.smil_last_error()
    t = _lib.MeshTopology()
    t.V, t.E, t.Q = 4, 6, 0
    assert lib.smil_mesh_regularisers(ctypes.byref(t), dummy, 1, 1, dummy, None, None, None, dummy, None) == -1
    assert b"topology tables missing" in lib.smil_last_error()
    assert lib.smil_mesh_regularisers(ctypes.byref(t), dummy, 1, 9, dummy, None, None, None, dummy, None) == -1
    assert b"terms" in lib.smil_last_error()
    assert lib.smil_mesh_reg_workspace_bytes(None, 1) == 0


def test_python_layer_raises_for_out_of_scope_options():
    from smilify_amd import fit3d

    x = torch.zeros(1, 4, 3)
    for kw in (dict(norm=1), dict(x_lengths=torch.tensor([4])), dict(point_reduction=None), dict(x_normals=x)):
        try:
            fit3d.chamfer_distance(x, x, **kw)
        except NotImplementedError:
            pass
        else:
            raise AssertionError(kw)
    try:
        fit3d.mesh_laplacian_smoothing(None, method="cot")
    except NotImplementedError:
        pass
    else:
        raise AssertionError("cot accepted")
    assert set(fit3d.SMALParamGroup.param_map) == {"init", "init_rot_lock", "init_rot_lock_trans", "init_rot_lock_trans_scale", "default",
                                                    "default_with_betas_trans", "shape", "pose", "deform", "all"}


# ---- the references of tests/test_gpu_mesh3d_kernels.py, pinned without a GPU ------------------------------------------------------
def test_philox_known_answers():
    """The three known-answer vectors of philox4x32-10 published with Random123 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for c, k, want in kat:
        assert tuple(int(v) for v in ref.philox4x32_10(c, k)) == want
    # arrays give what scalars give, element by element
    cs = [np.array([c[i] for c, _, _ in kat], np.uint64) for i in range(4)]
    ks = [np.array([k[i] for _, k, _ in kat], np.uint64) for i in range(2)]
    out = ref.philox4x32_10(cs, ks)
    assert [tuple(int(o[j]) for o in out) for j in range(3)] == [w for _, _, w in kat]


def test_sampler_restatement_properties():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [2, 3, 0], [9, 9, 9]], np.float32)
    f = np.array([[0, 0, 1], [0, 1, 2], [2, 2, 2], [3, 4, 5], [6, 6, 6], [6, 6, 6]])  # mesh 0: faces 0-3, mesh 1: no area, mesh 2: none
    off = np.array([0, 4, 6, 6])
    cum = np.array([0, 0.25, 0.25, 1.0, 0, 0])
    S = 4000
    pts, face, fmax = ref.sample_points(v, f, off, cum, S, seed=(5 << 32) | 9)
    assert (face[1:] == -1).all() and (pts[1:] == 0).all()
    assert set(np.unique(face[0]).tolist()) == {1, 3}
    n3 = int((face[0] == 3).sum())
    assert abs(n3 - 0.75 * S) <= 5 * np.sqrt(S * 0.75 * 0.25), n3
    assert (fmax[0][face[0] == 1] == 1).all() and (fmax[0][face[0] == 3] == 3).all()
    # inside the chosen triangle: z = 0, and face 1's points have x, y >= 0, x + y <= 1
    p1 = pts[0][face[0] == 1]
    assert (pts[0][:, 2] == 0).all() and (p1 >= 0).all() and (p1[:, 0] + p1[:, 1] <= 1 + 1e-7).all()
    # the seed's two halves, the mesh index and the sample index all enter the stream
    uf = [ref.sample_draws(n, 8, seed)[0] for n, seed in ((0, 9), (0, 9 | (1 << 32)), (1, 9), (0, 10))]
    assert all(not np.array_equal(uf[0], u) for u in uf[1:]) and len(np.unique(uf[0])) == 8
    uf, u, w = ref.sample_draws(2, 1000, 77)
    assert uf.dtype == np.float64 and u.dtype == np.float32 and (uf >= 0).all() and (uf < 1).all() and (u < 1).all() and (w < 1).all()
    assert (np.modf(uf * 2.0 ** 32)[0] != 0).any()  # more than 32 bits in the face uniform


def test_dyadic_grid_inputs_are_exact_and_tied():
    for N, P1, P2, sd, splits in ref.DYADIC_SHAPES:
        assert ref.chamfer_splits(N, P1, P2, sd) == splits, (N, P1, P2, sd)
        x, y = ref.dyadic_clouds(N, P1, P2)
        assert x.dtype == np.float32 and (x * 8 == np.round(x * 8)).all() and np.abs(x).max() <= 1 and np.abs(y).max() <= 1
        r = ref.dyadic_reference(N, P1, P2)
        assert (r["dx"] * 64 == np.round(r["dx"] * 64)).all() and (r["dx"].sum() + r["dy"].sum()) * 64 < 2 ** 24
        if min(P1, P2) >= ref.TIE_QUOTA_MIN_P:
            assert ref.tie_fraction(r, sd) >= 0.10, (N, P1, P2, ref.tie_fraction(r, sd))
        # numpy's first-occurrence rule: no smaller index is as near
        n, q = 0, P1 // 2
        d = ((x[n, q].astype(np.float64) - y[n].astype(np.float64)) ** 2).sum(-1)
        assert d[r["ix"][n, q]] == d.min() == r["dx"][n, q] and (d[:r["ix"][n, q]] > d.min()).all()
        assert (d == d.min()).sum() == r["nx"][n, q]
    assert ref.chamfer_chunk(4100, 4) == 1280 and ref.chamfer_chunk(5000, 3) == 1792 and ref.chamfer_chunk(1, 1) == 256


def test_chamfer_brute_and_chamfer_at_agree_with_chamfer():
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(3, 40, 3, generator=g, dtype=torch.float64), torch.randn(3, 55, 3, generator=g, dtype=torch.float64)
    r = ref.chamfer_brute(x.numpy(), y.numpy())
    for sd in (False, True):
        for ps in (False, True):
            for bs in (False, True):
                loss, ix, iy = ref.chamfer(x, y, sd, ps, bs)
                assert np.array_equal(r["ix"], ix.numpy()) and np.array_equal(r["iy"], iy.numpy())
                assert abs(ref.chamfer_loss_from(r["dx"], r["dy"], sd, ps, bs) - float(loss)) <= 1e-12 * float(loss)
                xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
                at = ref.chamfer_at(xr, yr, ix, iy, sd, ps, bs)
                assert abs(float(at.detach()) - float(loss)) <= 1e-12 * float(loss), (sd, ps, bs)
                gx, gy = torch.autograd.grad(at, (xr, yr))
                ox, sx, oy, sy = ref.chamfer_grad_parts(x.numpy(), y.numpy(), r["ix"], r["iy"], sd, ps, bs)
                assert np.abs(ox + sx - gx.numpy()).max() <= 1e-12 * float(gx.abs().max())
                assert np.abs(oy + sy - gy.numpy()).max() <= 1e-12 * float(gy.abs().max())
                if sd:
                    assert (oy == 0).all() and (sx == 0).all()


def test_hand_meshes_sparse_against_dense_laplacian_and_known_answers():
    from smilify_amd.mesh3d import Topology

    meshes = ref.hand_meshes()
    assert [len(meshes[k][0]) for k in ("grid_15x17", "grid_16x16", "grid_16x16_plus_1")] == [255, 256, 257]
    for name, (v, f) in meshes.items():
        assert v.dtype == np.float32
        vb = torch.from_numpy(v).double()[None] * torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)[:, None, None]
        ls, gs = ref.with_grad(ref.laplacian_loss_sparse, vb, f)
        ld, gd = ref.with_grad(ref.laplacian_loss, vb, f)
        assert abs(ls - ld) <= 1e-12 * max(ld, 1.0), name
        if name != "flat_grid_5x5":  # (there the dense form's 1/deg products leave residuals of 1e-16 whose direction is noise)
            assert (gs - gd).abs().max() <= 1e-9 * gd.abs().max(), name
        assert torch.isfinite(gs).all(), name
        T = Topology(f, len(v))
        assert np.array_equal(T.edges, ref.edges_brute(f)) and T.Q == len(ref.normal_pairs_brute(f)), name
    T = Topology(meshes["triangle"][1], 3)
    assert (T.E, T.Q) == (3, 0)
    T = Topology(meshes["three_on_edge"][1], 5)
    assert T.Q == 3
    roles = {i: sorted((T.vpair[T.vpair_ptr[i]:T.vpair_ptr[i + 1]] & 3).tolist()) for i in range(5)}
    assert roles[0] == [0, 0, 0] and roles[1] == [1, 1, 1] and sorted(sum((roles[i] for i in (2, 3, 4)), [])) == [2, 2, 2, 3, 3, 3]
    assert any(2 in roles[i] and 3 in roles[i] for i in (2, 3, 4))
    T = Topology(meshes["grid_16x16"][1], 256)
    assert T.E > 2 * 256 and T.Q > 2 * 256  # the block count of k_mesh_reg comes from E
    T = Topology(meshes["isolated"][1], 6)
    assert T.deg[4] == T.deg[5] == 0 and T.inv_deg[4] == 0
    # closed forms of the float64 reference
    one = lambda name, fn: float(fn(torch.from_numpy(meshes[name][0]).double()[None], meshes[name][1]))  # noqa: E731
    assert one("triangle", ref.normal_loss) == 0.0 and abs(one("triangle", ref.edge_loss) - 4.0 / 3.0) < 1e-12
    assert abs(one("tetrahedron", ref.edge_loss) - 1.5) < 1e-12
    assert abs(one("folded", ref.normal_loss) - (1 - ref.FOLD_COS / np.hypot(ref.FOLD_COS, ref.FOLD_SIN))) < 1e-12
    v = meshes["isolated"][0].astype(np.float64)
    lap_iso = one("isolated", ref.laplacian_loss_sparse)
    lap_tet = float(ref.laplacian_loss_sparse(torch.from_numpy(v[:4])[None], meshes["isolated"][1]))
    assert abs(lap_iso * 6 - (lap_tet * 4 + 0.0 + np.linalg.norm(v[5]))) < 1e-12  # rows of unreferenced vertices are -v_i
    # the flat grid's interior residuals are exactly 0 in the sparse float64 reference, and its gradient there is autograd's 0
    v, f = meshes["flat_grid_5x5"]
    vv = torch.from_numpy(v).double()[None]
    e = torch.from_numpy(ref.edges_brute(f))
    rows, cols = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
    deg = torch.bincount(rows, minlength=25).double()
    r = torch.zeros_like(vv).index_add_(1, rows, vv[:, cols]) * (1.0 / deg)[None, :, None] - vv  # as laplacian_loss_sparse
    interior = [i * 5 + j for i in range(1, 4) for j in range(1, 4)]
    assert (r[0, interior] == 0).all()
    # a face with a zero normal: torch divides each vector by max(|n|, 1e-8), so the pair's term is 1 and its gradient is finite
    l, g = ref.with_grad(ref.normal_loss, torch.from_numpy(meshes["zero_normal"][0])[None], meshes["zero_normal"][1])
    assert np.isfinite(l) and torch.isfinite(g).all() and float(g.abs().max()) > 1e6
    a = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
    b = torch.tensor([[0.0, 0, 2]], dtype=torch.float64)
    c = torch.cosine_similarity(a, b, dim=-1)
    assert float(c.detach()) == 0.0 and torch.equal(torch.autograd.grad(c.sum(), a)[0], torch.tensor([[0.0, 0, 1e8]], dtype=torch.float64))
