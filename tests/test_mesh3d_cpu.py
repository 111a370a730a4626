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
