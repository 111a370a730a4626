"""CPU side of the 3-D alignment (smilify_amd.align): the float64 restatement tests/align_ref.py pinned to hand-worked cases and to its
own finite differences, the conditions of the case sets tests/align_cases.py, argument validation before any device, and what the
robust variant is for - the outlier set."""
import math

import pytest
import torch

import align_cases as cases
import align_ref as ref

F64 = dict(dtype=torch.float64)
CROSS = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 2.0, 0], [0, -2.0, 0], [0, 0, 3.0], [0, 0, -3.0]], **F64)  # vx = 2 + 8 + 18 = 28


def test_identity_by_hand():
    src = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 1]], **F64)[None]
    x, w = ref.similarity_transform(src, src.clone())
    assert x.status.tolist() == [ref.OK]
    assert torch.allclose(x.R[0], torch.eye(3, **F64), atol=1e-14) and torch.allclose(x.t[0], torch.zeros(3, **F64), atol=1e-14)
    assert abs(float(x.s[0]) - 1.0) < 1e-14 and float(x.rms[0]) < 1e-14
    assert torch.equal(w, torch.ones(1, 5, **F64))


def test_quarter_turn_with_shift_and_scale_by_hand():
    """dst = 2.5 Rz(90 deg) src + (1, -2, 3): (x, y, z) -> (-2.5 y + 1, 2.5 x - 2, 2.5 z + 3)."""
    src = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 2, 1]], **F64)
    dst = torch.stack([-2.5 * src[:, 1] + 1.0, 2.5 * src[:, 0] - 2.0, 2.5 * src[:, 2] + 3.0], 1)
    x, _ = ref.similarity_transform(src[None], dst[None], weights=torch.tensor([1.0, 2.0, 0.5, 1.0, 3.0], **F64))
    want = torch.tensor([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]], **F64)
    assert x.status.tolist() == [ref.OK]
    assert torch.allclose(x.R[0], want, atol=1e-14) and torch.allclose(x.t[0], torch.tensor([1.0, -2.0, 3.0], **F64), atol=1e-13)
    assert abs(float(x.s[0]) - 2.5) < 1e-14 and float(x.rms[0]) < 1e-13
    rigid, _ = ref.rigid_transform(src[None], dst[None])
    assert torch.allclose(rigid.R[0], want, atol=1e-14) and float(rigid.s[0]) == 1.0 and float(rigid.rms[0]) > 0.1


def test_mirrored_cloud_by_hand():
    """The cross mirrored in x: M = diag(-2, 8, 18).  Over proper rotations sum_ab R[a][b] M[b][a] is largest at R = I (24, against 12 and
    -8 for the two half turns that flip x): no reflection comes back, s = 24 / 28 and rms^2 = (vy - 24^2 / 28) / 6."""
    dst = CROSS * torch.tensor([-1.0, 1.0, 1.0], **F64)
    x, _ = ref.similarity_transform(CROSS[None], dst[None])
    assert x.status.tolist() == [ref.OK]
    assert torch.allclose(x.R[0], torch.eye(3, **F64), atol=1e-14) and abs(float(torch.linalg.det(x.R[0])) - 1.0) < 1e-14
    assert abs(float(x.s[0]) - 24.0 / 28.0) < 1e-14 and torch.allclose(x.t[0], torch.zeros(3, **F64), atol=1e-14)
    assert abs(float(x.rms[0]) - math.sqrt((28.0 - 24.0 ** 2 / 28.0) / 6.0)) < 1e-14
    # Horn's matrix of diag(-2, 8, 18): diagonal (24, -28, -8, 12), gap = (24 - 12) / max(24, 28)
    assert abs(float(x.gap[0]) - 12.0 / 28.0) < 1e-14


def test_horn_matrix_is_the_quadratic_form_of_the_rotation():
    """q^T N(M) q = sum_ab R(q)[a][b] M[b][a] for a unit quaternion q: what makes the top eigenvector the best rotation."""
    g = torch.Generator().manual_seed(3)
    M = torch.randn(3, 3, generator=g, **F64)
    q = torch.nn.functional.normalize(torch.randn(4, generator=g, **F64), dim=0)
    a, b, c, d = q.tolist()
    R = torch.tensor([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                      [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                      [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]], **F64)
    assert abs(float(q @ ref.horn_matrix(M) @ q) - float((R * M.T).sum())) < 1e-14


@pytest.mark.parametrize("with_scale", [True, False])
def test_gradcheck_of_the_restatement(with_scale):
    c = cases.regular(2, 6, 3)

    def f(s, d):
        x, _ = ref.similarity_transform(s, d, weights=c["weights"], mask=c["mask"], with_scale=with_scale)
        return torch.cat([x.R.reshape(-1), x.t.reshape(-1), x.s.reshape(-1)])

    assert torch.autograd.gradcheck(f, (c["src"].clone().requires_grad_(), c["dst"].clone().requires_grad_()), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_degenerate_problems_have_zero_gradients_in_the_restatement():
    for name, c, status in cases.degenerate():
        x, _, g = ref.value_and_grads(c["src"], c["dst"], cases.probes(1, 1), weights=c["weights"], mask=c["mask"])
        assert x.status.tolist() == [status], name
        assert torch.equal(x.R[0], torch.eye(3, **F64)) and float(x.s[0]) == 1.0, name
        assert not g["src"].any() and not g["dst"].any(), name
        if status == ref.EMPTY:
            assert not x.t.any() and float(x.rms[0]) == 0.0, name


@pytest.mark.parametrize("B,J", [(1, 4), (3, 63), (65, 64), (3, 65), (65, 130)])
@pytest.mark.parametrize("weights", ["BJ", "J", None])
def test_regular_set_meets_its_conditions(B, J, weights):
    c = cases.regular(B, J, seed=J, weights=weights)
    cases.check_regular(**c)
    # ... and still does once the points have passed through float32 storage
    cases.check_regular(c["src"].float().double(), c["dst"].float().double(), c["weights"], c["mask"])
    x, _ = ref.similarity_transform(c["src"], c["dst"], weights=c["weights"], mask=c["mask"])
    assert float((torch.linalg.det(x.R) - 1.0).abs().max()) < 1e-12, "a mirrored target must still get a proper rotation"
    if weights == "BJ" and J > 6:
        assert bool((c["weights"] == 0).any()) and bool((c["mask"] == 0).any())


def test_wave_edge_sets_below_four_points():
    three = cases.wave_edge(65, 3, seed=3)
    x, _ = ref.similarity_transform(three["src"], three["dst"], weights=three["weights"], mask=three["mask"])
    assert bool((x.status == ref.OK).all()) and float(x.gap.min()) >= cases.MIN_GAP_REGULAR
    for J, status in ((0, ref.EMPTY), (1, ref.DEGENERATE), (2, ref.DEGENERATE)):
        c = cases.wave_edge(3, J, seed=J)
        x, _ = ref.similarity_transform(c["src"], c["dst"], weights=c["weights"], mask=c["mask"])
        assert x.status.tolist() == [status] * 3


def test_dropped_joints_in_the_restatement():
    c = cases.with_nan()
    x, w = ref.similarity_transform(c["src"], c["dst"])
    assert x.status.tolist() == [ref.OK] and float(w[0, 2]) == 0.0 and float(w[0, 5]) == 0.0 and int((w > 0).sum()) == 7
    keep = [j for j in range(9) if j not in (2, 5)]
    y, _ = ref.similarity_transform(c["src"][:, keep], c["dst"][:, keep])
    assert torch.equal(x.R, y.R) and torch.equal(x.t, y.t) and torch.equal(x.s, y.s)


def test_outlier_set_on_the_restatement():
    """What the robust variant is for.  J = 30, noise 0.01, six joints displaced by N(0, 5^2), seeds 0 to 49: with 10 reweighted solves at
    robust_scale 0.05 every seed recovers the true transform within 0.05 (largest coordinate difference of the moved src points); the
    plain solve misses it by at least 0.5 on every seed.  Measured: at most 0.034 robust, at least 0.60 plain."""
    robust, plain = [], []
    for seed in range(50):
        c = cases.outliers(seed)
        assert c["src"].shape == (1, 30, 3) and len(set(c["idx"].tolist())) == 6
        xr, w = ref.similarity_transform(c["src"], c["dst"], robust_iters=10, robust_scale=0.05)
        xp, _ = ref.similarity_transform(c["src"], c["dst"])
        robust.append(cases.transform_error(xr, c))
        plain.append(cases.transform_error(xp, c))
        assert float(w[0, c["idx"]].max()) < 0.2, "the displaced joints lose their weight"
    print(f"outlier set: robust max {max(robust):.3g}, plain min {min(plain):.3g}")
    assert max(robust) <= 0.05
    assert min(plain) >= 0.5


def test_joint_errors_restatement_by_hand():
    pred = torch.tensor([[[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [float("nan"), 0, 0]]], **F64)
    target = torch.tensor([[[1.0, 0, 3], [0, 1, 4], [0, 0, 0], [5, 5, 5], [1, 1, 1]]], **F64)
    dist, valid, status = ref.joint_errors(pred, target, mask=torch.tensor([[1, 1, 1, 0, 1]]), scale=2.0)
    assert valid.tolist() == [[True, True, False, False, False]]  # the sentinel, the masked joint and the NaN drop out
    assert dist.tolist() == [[6.0, 8.0, 0.0, 0.0, 0.0]] and status.tolist() == [ref.OK]
    assert float(ref.pooled(dist, valid)) == 7.0
    dist, valid, _ = ref.joint_errors(pred, target, sentinel=False)
    assert valid.tolist() == [[True, True, True, True, False]] and dist.tolist() == [[3.0, 4.0, 1.0, 0.0, 0.0]]
    none = ref.joint_errors(pred, target, mask=torch.zeros(1, 5))
    assert none[2].tolist() == [ref.EMPTY] and float(ref.pooled(none[0], none[1])) == 0.0


# ---- argument validation: nothing below needs a device -----------------------------------------------------------------------------
def test_argument_validation_without_a_device():
    from smilify_amd import _lib, align

    src, dst = torch.zeros(2, 5, 3), torch.zeros(2, 5, 3)
    bad = [
        dict(src=torch.zeros(2, 5, 2)), dict(src=torch.zeros(5)), dict(dst=torch.zeros(2, 4, 3)), dict(dst=torch.zeros(5, 3)),
        dict(src=src.half()), dict(dst=dst.double()), dict(src=src.tolist()),
        dict(weights=torch.ones(4)), dict(weights=torch.ones(2, 5, 1)), dict(weights=torch.ones(5, dtype=torch.bool)),
        dict(weights=torch.tensor([1.0, -1.0, 1, 1, 1])), dict(weights=torch.tensor([1.0, float("nan"), 1, 1, 1])),
        dict(weights=torch.tensor([1.0, float("inf"), 1, 1, 1])),
        dict(mask=torch.ones(2, 4)), dict(mask=[1, 1]),
        dict(min_gap=-1e-3), dict(min_gap=float("nan")), dict(min_gap=float("inf")),
        dict(robust_iters=-1), dict(robust_iters=2), dict(robust_iters=2, robust_scale=0.0), dict(robust_iters=2, robust_scale=-1.0),
        dict(robust_iters=2, robust_scale=float("nan")), dict(robust_scale=float("inf")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            align.similarity_transform(**dict(dict(src=src, dst=dst), **kw))
    with pytest.raises(ValueError):
        align.rigid_transform(src, dst, min_gap=-1.0)
    for kw in (dict(align="affine"), dict(scale=float("nan")), dict(min_gap=-1.0), dict(mask=torch.ones(2, 4))):
        with pytest.raises(ValueError):
            align.joint_errors(src, dst, **kw)
    with pytest.raises(ValueError):
        align.global_pose_from_alignment(None, torch.zeros(2, 3), torch.zeros(2, 3))
    # well-formed arguments on the CPU: there is no CPU path
    for call in (lambda: align.similarity_transform(src, dst), lambda: align.rigid_transform(src[0], dst[0]),
                 lambda: align.similarity_transform(src, dst, weights=torch.ones(5), mask=torch.ones(2, 5)),
                 lambda: align.joint_errors(src, dst), lambda: align.pa_mpjpe(src, dst), lambda: align.mpjpe(src, dst)):
        with pytest.raises(_lib.SmilError):
            call()


def test_library_refuses_bad_scalars_without_a_device():
    from smilify_amd import _lib

    lib = _lib.load()
    fwd = lambda **kw: lib.smil_align_forward(None, None, None, kw.get("rows", 0), None, kw.get("B", 1), kw.get("J", 1), 1,  # noqa: E731
                                              kw.get("min_gap", 1e-10), kw.get("iters", 0), kw.get("f", 1.0), kw.get("dtype", _lib.ROT_F64),
                                              *([None] * 9))
    for kw, text in ((dict(min_gap=-1.0), b"min_gap"), (dict(min_gap=float("nan")), b"min_gap"), (dict(min_gap=float("inf")), b"min_gap"),
                     (dict(iters=1, f=0.0), b"robust_scale"), (dict(iters=1, f=float("inf")), b"robust_scale"), (dict(iters=-1), b"robust_iters"),
                     (dict(B=-1), b"negative"), (dict(J=-1), b"negative"), (dict(dtype=7), b"dtype"), (dict(rows=2), b"weight_rows"),
                     (dict(), b"null")):
        assert fwd(**kw) == -1, kw
        assert text in lib.smil_last_error(), (kw, lib.smil_last_error())
    assert fwd(B=0) == 0  # an empty batch succeeds without a launch
    err = lambda **kw: lib.smil_align_errors(None, None, None, kw.get("B", 1), 1, kw.get("mode", 0), 1, kw.get("scale", 1.0),  # noqa: E731
                                             kw.get("min_gap", 1e-10), _lib.ROT_F32, None, None, None, None)
    for kw in (dict(mode=3), dict(scale=float("nan")), dict(min_gap=-1.0), dict()):
        assert err(**kw) == -1, kw
    assert err(B=0) == 0
    assert lib.smil_align_backward(*([None] * 8), -1, 1, 1, _lib.ROT_F32, None, None, None) == -1
    assert lib.smil_align_backward(*([None] * 8), 0, 1, 1, _lib.ROT_F32, None, None, None) == 0
