"""CPU-side checks of the rotation conversions: the float64 restatement (tests/rotations_ref.py) against scipy's independent statement
of the maps and against the edge facts the kernels are specified by, the library's argument validation, and the public module's
refusal of what it does not support.  The kernels themselves are compared with the restatement in tests/test_gpu_rotations.py."""
import ctypes

import pytest
import torch

import rotations_cases as cases
import rotations_ref as ref

F64 = torch.float64


def test_restatement_matches_scipy_fixture(golden):
    g = golden("rotations_ref")
    aa, matrix, rotvec = (torch.from_numpy(g[k]) for k in ("aa", "matrix", "rotvec"))
    n_regular = int(g["n_regular"])
    # the fixture's inputs are the case sets' own (the generator is still the one that wrote it)
    assert torch.equal(aa[:n_regular], cases.regular(n_regular)["aa"]) and torch.equal(aa[n_regular:], cases.small_angle()["aa"])
    assert float((ref.axis_angle_to_matrix(aa) - matrix).abs().max()) <= 1e-12
    assert float((ref.matrix_to_axis_angle(matrix) - rotvec).abs().max()) <= 1e-12
    assert float((ref.matrix_to_axis_angle(ref.axis_angle_to_matrix(aa)) - aa).abs().max()) <= 1e-12
    # 6-D: the first two rows of a rotation matrix give the matrix back; the slice is the inverse map
    assert float((ref.rotation_6d_to_matrix(ref.matrix_to_rotation_6d(matrix)) - matrix).abs().max()) <= 1e-12
    assert torch.equal(ref.matrix_to_rotation_6d(matrix), matrix[:, :2].reshape(-1, 6))
    assert float((ref.rotation_6d_to_axis_angle(ref.axis_angle_to_rotation_6d(aa)) - aa).abs().max()) <= 1e-12


def test_regular_set_is_regular():
    """The seed's rows lie in the stated ranges, as float64 and after the cast to float32 (what the float32 GPU tests feed)."""
    c = cases.regular(257)
    cases.check_regular(d6=c["d6"], aa=c["aa"])
    cases.check_regular(R=c["R"])
    cases.check_regular(d6=c["d6"].float(), aa=c["aa"].float())
    cases.check_regular(R=c["R"].float())
    big = cases.regular(2048 * 256 + 1)  # the size of the stride-loop test
    cases.check_regular(d6=big["d6"].float(), R=big["R"].float(), aa=big["aa"].float())
    p, t, q, near = cases.distance_pairs(257)
    for a, b in ((q, near), (q.float(), near.float())):
        d = ref.rotation_6d_distance(a.double(), b.double())
        assert cases.NEAR_DISTANCE[0] <= float(d.min()) and float(d.max()) <= cases.NEAR_DISTANCE[1]


def test_degenerate_6d_rows():
    d = cases.degenerate_6d()
    R = ref.rotation_6d_to_matrix(d)
    assert torch.equal(R[0], torch.zeros(3, 3, dtype=F64))
    for row in (1, 2, 7):  # a2 parallel to a1: b2 = b3 = 0
        assert torch.equal(R[row, 1:], torch.zeros(2, 3, dtype=F64)) and float(R[row, 0].norm()) == 1.0
    assert torch.equal(R[3, 0], torch.tensor([0.1, 0.0, 0.0], dtype=F64))  # (1e-13, 0, 0) / 1e-12
    assert torch.equal(R[5, 1], torch.tensor([0.0, 0.1, 0.0], dtype=F64))
    assert torch.equal(R[6, 0], torch.zeros(3, dtype=F64)) and torch.equal(R[6, 2], torch.zeros(3, dtype=F64))
    assert torch.equal(R[8], torch.tensor([[0.0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=F64))
    assert torch.equal(R[9, 1:], torch.zeros(2, 3, dtype=F64))
    # the clamp makes gradients of order 1e12: finite
    x = d.clone().requires_grad_(True)
    (ref.rotation_6d_to_matrix(x) * cases.weights((10, 3, 3), 3)).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and 1e11 < float(x.grad.abs().max()) < 1e13


def test_jacobians_at_identity_and_zero():
    m = torch.eye(3, dtype=F64).requires_grad_(True)
    aa = ref.matrix_to_axis_angle(m)
    assert torch.equal(aa.detach(), torch.zeros(3, dtype=F64))
    J = torch.stack([torch.autograd.grad(aa[k], m, retain_graph=True)[0] for k in range(3)])
    assert bool(torch.isfinite(J).all())
    assert float(J[0, 2, 1]) == 0.5 and float(J[0, 1, 2]) == -0.5 and float(J[1, 0, 2]) == 0.5 and float(J[2, 1, 0]) == 0.5
    a = torch.zeros(3, dtype=F64, requires_grad=True)
    R = ref.axis_angle_to_matrix(a)
    assert torch.equal(R.detach(), torch.eye(3, dtype=F64))
    J = torch.stack([torch.autograd.grad(R.reshape(9)[k], a, retain_graph=True)[0] for k in range(9)]).reshape(3, 3, 3)
    assert bool(torch.isfinite(J).all())
    assert float(J[2, 1, 0]) == 1.0 and float(J[1, 2, 0]) == -1.0 and float(J[0, 2, 1]) == 1.0 and float(J[1, 0, 2]) == 1.0


def test_zero_distance_has_zero_gradient():
    p = cases.regular(8)["d6"].requires_grad_(True)
    t = p.detach().clone().requires_grad_(True)
    d = ref.rotation_6d_distance(p, t)
    assert torch.equal(d.detach(), torch.zeros(8, dtype=F64))
    d.sum().backward()
    assert torch.equal(p.grad, torch.zeros_like(p)) and torch.equal(t.grad, torch.zeros_like(t))


def test_visibility_loss_formula():
    p, t, _, _ = cases.distance_pairs(6)
    vis = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0], dtype=F64)
    d = ref.rotation_6d_distance(p, t)
    want = (d[0] + d[2] + d[3]) / (3 + 1e-8) + 1e-8
    assert float(ref.visibility_weighted_rotation_loss(p, t, vis)) == pytest.approx(float(want), rel=1e-15)
    none = ref.visibility_weighted_rotation_loss(p.requires_grad_(True), t, torch.zeros(6))
    assert float(none.detach()) == 1e-8 and none.is_leaf


def test_gradcheck_of_the_restatement():
    c = cases.regular(5)
    for fn, x in ((ref.rotation_6d_to_matrix, c["d6"]), (ref.axis_angle_to_matrix, c["aa"]), (ref.matrix_to_axis_angle, c["R"]),
                  (ref.rotation_6d_to_axis_angle, c["d6"])):
        assert torch.autograd.gradcheck(fn, (x.clone().requires_grad_(True),), eps=1e-6, atol=1e-6, rtol=1e-5)
    p, t, _, _ = cases.distance_pairs(5)
    assert torch.autograd.gradcheck(ref.rotation_6d_distance, (p.requires_grad_(True), t.requires_grad_(True)), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- the C ABI without a GPU ----
FORWARD = ("smil_rot6d_to_matrix", "smil_axis_angle_to_matrix", "smil_matrix_to_axis_angle", "smil_rot6d_to_axis_angle")
BACKWARD = ("smil_rot6d_to_matrix_backward", "smil_axis_angle_to_matrix_backward", "smil_matrix_to_axis_angle_backward", "smil_rot6d_distance")


def _entry_points():
    """(name, callable(pointers..., n, dtype), number of required pointers): a host buffer stands in for device memory - every call
    here is refused, or returns, before anything is launched."""
    from smilify_amd import _lib

    lib = _lib.load()
    for name in FORWARD:
        yield name, getattr(lib, name), 2
    for name in BACKWARD:
        yield name, getattr(lib, name), 3
    yield "smil_rot6d_distance_backward", lambda a, b, c, n, dt, s: lib.smil_rot6d_distance_backward(a, b, c, None, None, n, dt, s), 3


def test_abi_argument_validation_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name, fn, k in _entry_points():
        ok = [p] * k
        assert fn(*ok, -1, _lib.ROT_F32, None) == -1 and name.encode() in lib.smil_last_error() and b"negative" in lib.smil_last_error()
        assert fn(*ok, 1, 2, None) == -1 and name.encode() in lib.smil_last_error() and b"dtype" in lib.smil_last_error()
        assert fn(*ok, 1, -1, None) == -1
        for missing in range(k):
            args = list(ok)
            args[missing] = None
            assert fn(*args, 1, _lib.ROT_F64, None) == -1 and name.encode() in lib.smil_last_error() and b"null" in lib.smil_last_error()
        assert fn(*ok, 0, _lib.ROT_F32, None) == 0
        assert fn(*([None] * k), 0, _lib.ROT_F64, None) == 0  # an empty tensor has no storage


def test_public_module_refuses_cpu_tensors_and_other_dtypes():
    from smilify_amd import _lib, rotations

    d6, aa, R = torch.zeros(2, 6), torch.zeros(2, 3), torch.eye(3).expand(2, 3, 3)
    for fn, x in ((rotations.rotation_6d_to_matrix, d6), (rotations.axis_angle_to_matrix, aa), (rotations.matrix_to_axis_angle, R),
                  (rotations.rotation_6d_to_axis_angle, d6), (rotations.axis_angle_to_rotation_6d, aa)):
        with pytest.raises(_lib.SmilError, match="GPU"):
            fn(x)
        with pytest.raises(TypeError, match="float32 and float64"):
            fn(x.half())
        with pytest.raises(TypeError, match="float32 and float64"):
            fn(x.long())
    with pytest.raises(_lib.SmilError, match="GPU"):
        rotations.rotation_6d_distance(d6, d6)
    with pytest.raises(TypeError):
        rotations.rotation_6d_distance(d6.half(), d6.half())
    with pytest.raises(_lib.SmilError, match="GPU"):
        rotations.visibility_weighted_rotation_loss(d6, d6, torch.ones(2))


def test_public_module_shape_errors_and_the_slice():
    from smilify_amd import rotations

    with pytest.raises(ValueError, match="Invalid rotation matrix shape"):
        rotations.matrix_to_axis_angle(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="Invalid rotation matrix shape"):
        rotations.matrix_to_rotation_6d(torch.zeros(3))
    with pytest.raises(ValueError):
        rotations.rotation_6d_to_matrix(torch.zeros(2, 5))
    with pytest.raises(ValueError):
        rotations.axis_angle_to_matrix(torch.zeros(2, 4))
    with pytest.raises(ValueError):
        rotations.rotation_6d_to_axis_angle(torch.zeros(6, 2))
    with pytest.raises(ValueError):
        rotations.rotation_6d_distance(torch.zeros(2, 6), torch.zeros(3, 6))
    # matrix_to_rotation_6d is plain torch: a copy of the first two rows, differentiable, on any device
    m = torch.arange(18.0).reshape(2, 3, 3).requires_grad_(True)
    d6 = rotations.matrix_to_rotation_6d(m)
    assert torch.equal(d6.detach(), ref.matrix_to_rotation_6d(m.detach())) and d6.shape == (2, 6)
    d6.sum().backward()
    assert torch.equal(m.grad[:, :2], torch.ones(2, 2, 3)) and torch.equal(m.grad[:, 2], torch.zeros(2, 3))
