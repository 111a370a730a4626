"""CPU checks of the SDF-guided term: the float64 restatement (tests/sdf_ref.py) against the reference's own SDF_distance
(tests/golden/sdf_distance_ref.npz, written by tests/golden/make_sdf_fixture.py), its analytic gradient against autograd, the C ABI's
argument validation, the Python layer's guard rails and the sampler's index map."""
import ctypes

import numpy as np
import pytest
import torch

import sdf_ref


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("sdf_distance_ref")


def _cases(g):
    for name in g["cases"].tolist():
        k, bsum, psum, single = (int(v) for v in g[name + "_cfg"])
        yield name, k, bool(bsum), bool(psum), bool(single)


def test_restatement_reproduces_the_reference(fixture):
    g = fixture
    names = [c[0] for c in _cases(g)]
    assert any("k50" in n for n in names) and any("k1" in n for n in names) and any("single" in n for n in names)
    for name, k, bsum, psum, single in _cases(g):
        loss, dx, dy, _, _ = sdf_ref.sdf_term(g["x"], g["y"], g["x_sdf"], g["y_sdf"], k, psum, bsum, single, with_grad=True)
        ref = float(g[name + "_loss"])
        assert abs(loss - ref) <= 1e-12 * abs(ref), (name, loss, ref)
        for got, want in ((dx, g[name + "_dx"]), (dy, g[name + "_dy"])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


def test_analytic_gradient_matches_autograd(fixture):
    g = fixture
    for k, psum, bsum, single in ((50, False, False, False), (7, True, False, True), (1, False, True, False)):
        _, dx, dy, ix, iy = sdf_ref.sdf_term(g["x"], g["y"], g["x_sdf"], g["y_sdf"], k, psum, bsum, single, with_grad=True)
        ax, ay = sdf_ref.sdf_grad_at(g["x"], g["y"], g["x_sdf"], g["y_sdf"], ix, iy, psum, bsum, single)
        assert np.abs(ax - dx).max() <= 1e-12 * np.abs(dx).max()
        assert np.abs(ay - dy).max() <= 1e-12 * np.abs(dy).max()


def test_knn_brute_orders_by_distance_then_index():
    q = np.zeros((1, 1, 3))
    c = np.array([[[1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0, 1], [0, 0, -1]]], np.float64)
    d, i, nxt = sdf_ref.knn_brute(q, c, 3)
    assert i.tolist() == [[[2, 0, 1]]] and d.tolist() == [[[0.25, 1.0, 1.0]]] and nxt.tolist() == [[1.0]]


def test_abi_rejects_bad_arguments():
    from smilify_amd import _lib

    lib = _lib.load()
    K_MAX = _lib.KNN_MAX_K
    assert K_MAX >= 64
    p = ctypes.c_void_p(256)  # never dereferenced: validation comes first
    assert lib.smil_knn(None, p, 1, 8, 8, 2, p, p, None, None, p, None) == -1 and b"null" in lib.smil_last_error()
    assert lib.smil_knn(p, p, 1, 8, 8, 2, p, p, p, None, p, None) == -1 and b"together" in lib.smil_last_error()
    for P1, P2, K in ((8, 8, 9), (8, 8, 0), (100, 100, K_MAX + 1)):
        assert lib.smil_knn(p, p, 1, P1, P2, K, p, p, None, None, p, None) == -1 and b"bad sizes" in lib.smil_last_error()
        assert lib.smil_knn_workspace_bytes(1, P1, P2, K) == 0
        assert lib.smil_sdf_distance_workspace_bytes(1, P1, P2, K) == 0
    assert lib.smil_knn(p, p, 1, 4, 8, 6, p, p, p, p, p, None) == -1 and b"bad sizes" in lib.smil_last_error()  # K > P1, both directions
    assert lib.smil_knn_workspace_bytes(1, 8, 8, 8) > 0 and lib.smil_sdf_distance_workspace_bytes(2, 70, 300, 50) > 0
    sdf = lambda *a: lib.smil_sdf_distance(*a)  # noqa: E731
    assert sdf(p, p, None, p, 1, 8, 8, 2, 0, 0, 0, p, None, None, None, None, None, None, p, None) == -1
    assert b"null" in lib.smil_last_error()
    for P1, P2, K in ((8, 8, 9), (8, 8, 0), (100, 100, K_MAX + 1), (1, 8, 1), (8, 1, 1)):
        assert sdf(p, p, p, p, 1, P1, P2, K, 0, 0, 0, p, None, None, None, None, None, None, p, None) == -1
        assert b"bad sizes" in lib.smil_last_error()
    assert lib.smil_sdf_distance_workspace_bytes(1, 1, 8, 1) == 0 and lib.smil_sdf_distance_workspace_bytes(1, 8, 1, 1) == 0
    assert sdf(p, p, p, p, 1, 8, 8, 2, 0, 0, 0, p, p, None, None, None, None, None, p, None) == -1
    assert b"together" in lib.smil_last_error()
    assert lib.smil_sample_vertices(None, p, p, 1, 4, 0, p, p, p, None) == -1 and b"null" in lib.smil_last_error()
    assert lib.smil_sample_vertices(p, p, p, 0, 4, 0, p, p, p, None) == -1 and b"bad sizes" in lib.smil_last_error()
    assert lib.smil_sample_vertices_backward(None, p, p, 4, 4, 1, 4, p, p, None) == -1
    assert lib.smil_sample_vertices_backward_workspace_bytes(0, 1) == 0


def test_python_layer_guard_rails():
    from smilify_amd import fit3d

    x, y = torch.zeros(1, 4, 3), torch.zeros(1, 6, 3)
    xs, ys = torch.zeros(1, 4), torch.zeros(1, 6)
    with pytest.raises(NotImplementedError):
        fit3d.SDF_distance(x, y, xs, ys, 2, norm=1)
    with pytest.raises(ValueError):
        fit3d.SDF_distance(x, y, xs, ys, 2, norm=3)
    with pytest.raises(NotImplementedError):
        fit3d.SDF_distance(x, y, xs, ys, 2, visualize=True)
    with pytest.raises(NotImplementedError):
        fit3d.SDF_distance(x, y, xs, ys, 2, point_reduction=None)
    with pytest.raises(ValueError):
        fit3d.SDF_distance(x, y, xs, ys[:, :5], 2)
    with pytest.raises(ValueError):
        fit3d.SDF_distance(x, y, xs, ys, 0)
    with pytest.raises(NotImplementedError):
        fit3d.knn_points(x, y, norm=1, K=2)
    with pytest.raises(NotImplementedError):
        fit3d.knn_points(x, y, lengths1=torch.tensor([4]), K=2)
    from smilify_amd import engine

    for fn in (lambda: engine.knn(x, y, 7), lambda: engine.knn(x, y, 0), lambda: engine.knn(x, y, 5, both=True),
               lambda: engine.sdf_distance(x, y, xs, ys, 5), lambda: engine.sdf_distance(x[:, :1], y, xs[:, :1], ys, 1),
               lambda: engine.knn(torch.zeros(1, 100, 3), torch.zeros(1, 100, 3), 65)):
        with pytest.raises(ValueError):  # sizes are checked before a device is asked for
            fn()


def test_parser_knows_the_sdf_flags():
    from smilify_amd import fit3d

    a = fit3d.build_parser().parse_args(["--mesh_dir", "m"])
    assert a.use_sdf is False and a.sdf_dir is None
    a = fit3d.build_parser().parse_args(["--mesh_dir", "m", "--use_sdf", "--sdf_dir", "d"])
    assert a.use_sdf is True and a.sdf_dir == "d"


def test_sdf_value_files(tmp_path):
    import pickle

    from smilify_amd import fit3d

    np.savez(tmp_path / "a_sdf.npz", vertex_sdf=np.arange(5, dtype=np.float64))
    with open(tmp_path / "b_sdf.pkl", "wb") as fh:
        pickle.dump({"vertex_sdf": torch.arange(3.0)}, fh)
    assert fit3d.load_sdf_values("a.obj", str(tmp_path), "cpu").tolist() == [0, 1, 2, 3, 4]
    assert fit3d.load_sdf_values("b", str(tmp_path), "cpu").tolist() == [0, 1, 2]
    assert fit3d.load_sdf_values("c.obj", str(tmp_path), "cpu") is None


def test_vertex_index_map_by_hand():
    assert sdf_ref.vertex_index(0, 3020) == 0
    assert sdf_ref.vertex_index(2 ** 32 - 1, 3020) == 3019
    assert sdf_ref.vertex_index(2 ** 32 - 1, 6) == 5
    assert sdf_ref.vertex_index(2 ** 31, 6) == 3
    for r in (0, 1, 12345, 2 ** 31, 2 ** 32 - 1):
        assert sdf_ref.vertex_index(r, 1) == 0
    idx = sdf_ref.vertex_indices(1, 300, (1 << 63) - 1, 6)
    assert idx.min() >= 0 and idx.max() <= 5 and len(set(idx.tolist())) == 6
