"""CPU-side checks of the keypoint losses: the float64 restatement (tests/keypoint_losses_ref.py) against hand-worked values and
against the conventions the suite already pins, the properties of the seeded case sets, and the public module's argument checks.
The kernels themselves are compared with the restatement in tests/test_gpu_keypoint_losses.py."""
import math

import pytest
import torch

import keypoint_losses_cases as cases
import keypoint_losses_ref as ref

F64 = torch.float64
EPS = 1e-8


def t64(x):
    return torch.tensor(x, dtype=F64)


# ---- hand-worked values --------------------------------------------------------------------------------------------------------
def hand_2d():
    """Two samples, J = 2.  Sample 0: joint 0 valid with error (0.1, -0.2), joint 1 invisible.  Sample 1: joint 0 has a target
    outside [0,1], joint 1 valid with error (0.3, 0.0)."""
    target = t64([[[0.5, 0.5], [0.2, 0.2]], [[1.5, 0.5], [0.25, 0.75]]])
    rendered = target + t64([[[0.1, -0.2], [0.7, 0.7]], [[0.3, 0.3], [0.3, 0.0]]])
    visibility = t64([[1.0, 0.0], [1.0, 1.0]])
    return rendered, target, visibility


def test_hand_worked_2d_every_reduction():
    rendered, target, visibility = hand_2d()
    e0, e1 = 0.1 ** 2 + 0.2 ** 2, 0.3 ** 2
    want = dict(pooled=(e0 + e1) / (2 * 2 + EPS) + EPS, valid_samples=(e0 / (2 + EPS) + e1 / (2 + EPS)) / 2 + EPS,
                samples=(e0 / (2 + EPS) + e1 / (2 + EPS)) / 2 + EPS)
    for reduction, value in want.items():
        assert abs(float(ref.keypoint_loss_2d(rendered, target, visibility, reduction=reduction)) - value) <= 1e-15, reduction
    # joint weights (3, 5): sample 0 counts joint 0 (weight 3), sample 1 joint 1 (weight 5)
    w = t64([3.0, 5.0])
    want = dict(pooled=(3 * e0 + 5 * e1) / (2 * 8 + EPS) + EPS, valid_samples=(3 * e0 / (6 + EPS) + 5 * e1 / (10 + EPS)) / 2 + EPS)
    for reduction, value in want.items():
        assert abs(float(ref.keypoint_loss_2d(rendered, target, visibility, w, reduction=reduction)) - value) <= 1e-15, reduction
    # a third, selected sample without a valid joint: it enters the "samples" mean and not the "valid_samples" mean
    r3 = torch.cat([rendered, rendered[:1]])
    t3 = torch.cat([target, target[:1]])
    v3 = torch.cat([visibility, torch.zeros(1, 2, dtype=F64)])
    s = e0 / (2 + EPS) + e1 / (2 + EPS)
    assert abs(float(ref.keypoint_loss_2d(r3, t3, v3, reduction="valid_samples")) - (s / 2 + EPS)) <= 1e-15
    assert abs(float(ref.keypoint_loss_2d(r3, t3, v3, reduction="samples")) - (s / 3 + EPS)) <= 1e-15
    assert abs(float(ref.keypoint_loss_2d(r3, t3, v3, reduction="pooled")) - ((e0 + e1) / (4 + EPS) + EPS)) <= 1e-15
    # a sample mask that drops sample 1
    m = t64([1.0, 0.0, 1.0])
    assert abs(float(ref.keypoint_loss_2d(r3, t3, v3, mask=m, reduction="samples")) - (e0 / (2 + EPS) / 2 + EPS)) <= 1e-15
    assert abs(float(ref.keypoint_loss_2d(r3, t3, v3, mask=m, reduction="valid_samples")) - (e0 / (2 + EPS) + EPS)) <= 1e-15


def test_hand_worked_edges():
    rendered, target, visibility = hand_2d()
    for reduction in ("pooled", "valid_samples", "samples"):
        # all-zero weights: 0 / (0 + eps) + eps
        assert float(ref.keypoint_loss_2d(rendered, target, visibility, torch.zeros(2, dtype=F64), reduction=reduction)) == 0.0 / (0.0 + EPS) + EPS
        # nothing valid: exactly 1e-8, and a zero gradient
        x = rendered.clone().requires_grad_(True)
        loss = ref.keypoint_loss_2d(x, target, torch.zeros(2, 2), reduction=reduction)
        assert float(loss.detach()) == 1e-8
        loss.backward()
        assert not bool(x.grad.any())
    # bounds are inclusive; a non-finite rendered coordinate counts as 0 and takes no gradient
    target = t64([[[0.0, 1.0], [math.nextafter(0.0, -1.0), 0.5], [0.5, math.nextafter(1.0, 2.0)]]])
    rendered = t64([[[float("nan"), 0.75], [0.1, 0.1], [0.1, 0.1]]]).requires_grad_(True)
    loss = ref.keypoint_loss_2d(rendered, target, torch.ones(1, 3))
    assert abs(float(loss.detach()) - ((0.0 - 0.0) ** 2 + 0.25 ** 2) / (2 + EPS) - EPS) <= 1e-15
    loss.backward()
    g = rendered.grad
    assert float(g[0, 0, 0]) == 0.0 and abs(float(g[0, 0, 1]) - 2 * -0.25 / (2 + EPS)) <= 1e-15 and not bool(g[0, 1:].any())


def test_hand_worked_3d():
    """J = 2 per sample: a sentinel row, a non-finite target, a non-finite prediction, one valid joint."""
    target = t64([[[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], [[float("inf"), 0.0, 1.0], [1.0, 1.0, 1.0]]])
    pred = t64([[[5.0, 5.0, 5.0], [1.5, 2.0, 2.0]], [[0.0, 0.0, 0.0], [float("nan"), 1.0, 1.0]]])
    vis = torch.ones(2, 2)
    e = 0.5 ** 2 + 1.0 ** 2
    assert abs(float(ref.keypoint_loss_3d(pred, target, vis)) - (e / (3 + EPS) + EPS)) <= 1e-15  # one valid sample
    assert abs(float(ref.keypoint_loss_3d(pred, target, vis, reduction="pooled")) - (e / (3 + EPS) + EPS)) <= 1e-15
    assert float(ref.keypoint_loss_3d(pred, target, torch.zeros(2, 2))) == 1e-8


def test_restatement_is_differentiable_where_the_cases_say():
    c = cases.regular(2, 3, 4, seed=5)
    w = cases.joint_weights(4)
    kw = dict(eps=1e-6, atol=1e-7, rtol=1e-5)
    proj = c["proj"].clone().requires_grad_(True)
    for reduction in ("pooled", "valid_samples", "samples"):
        assert torch.autograd.gradcheck(lambda x: ref.keypoint_loss_2d(x, c["target"], c["visibility"], w, None, reduction), (proj,), **kw)
    pred, target, vis = cases.points_3d(3, 4)
    assert torch.autograd.gradcheck(lambda x: ref.keypoint_loss_3d(x, target, vis, w), (pred.requires_grad_(True),), **kw)
    leaves = [c[k].clone().requires_grad_(True) for k in ("joints", "R", "T", "fov")]
    assert torch.autograd.gradcheck(lambda j, R, T, f: ref.project_joints_to_views(j, R, T, f, c["S"], c["aspect"]), leaves, **kw)
    assert torch.autograd.gradcheck(
        lambda j, R, T, f: ref.multiview_keypoint_loss(j, R, T, f, c["target"], c["visibility"], c["S"], c["aspect"], None, w), leaves, **kw)
    cams = leaves[1:]
    # (every joint seen by all views: a joint seen once has cond(M) ~ 1e6 and is no subject for finite differences)
    assert torch.autograd.gradcheck(lambda R, T, f: ref.triangulate_joints_dlt(c["observed"], None, R, T, f, c["S"], c["aspect"])[0], cams, **kw)
    assert torch.autograd.gradcheck(
        lambda R, T, f: ref.triangulation_consistency_loss(c["observed"], c["visibility"], c["joints"] + 0.05, R, T, f, c["S"], c["aspect"], None, w),
        cams, **kw)


# ---- the camera convention -----------------------------------------------------------------------------------------------------
def test_projection_of_an_axis_aligned_camera_by_hand():
    """R = I, T = (0, 0, 4): view space is world space moved 4 along z.  With fov 90 degrees k11 = 1; aspect 2 halves k00."""
    S = 100.0
    R, T = torch.eye(3, dtype=F64).reshape(1, 1, 3, 3), t64([[[0.0, 0.0, 4.0]]])
    fov, aspect = t64([[90.0]]), t64([[2.0]])
    joints = t64([[[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0, -1.0, 0.0]]])
    out = ref.project_joints_to_views(joints, R, T, fov, S, aspect)[0, 0]
    n = S + 1e-8
    want = t64([[50.0, 50.0], [50.0, 50.0],               # on the optical axis: the image centre
                [50.0, 50.0 - 50.0 * 0.5 * 1.0 / 4.0],    # +x in view space: towards smaller x in pixels (ndc_to_yx)
                [50.0 - 50.0 * 1.0 / 4.0, 50.0],          # +y: towards smaller y
                [50.0 + 50.0 * 1.0 / 4.0, 50.0 - 50.0 * 0.5 * 2.0 / 4.0]]) / n
    assert float((out - want).abs().max()) <= 1e-15
    assert abs(float(out[0, 0]) - 0.5) <= 1e-9 and abs(float(out[0, 1]) - 0.5) <= 1e-9
    assert float(out[2, 1]) < float(out[0, 1])
    # R and T composed by hand: a camera turned 90 degrees about y looks along world +x
    Ry = t64([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]).reshape(1, 1, 3, 3)  # v = X Ry: vz = x, vx = -z
    out = ref.project_joints_to_views(t64([[[0.0, 0.5, -1.0]]]), Ry, T, fov, S, None)[0, 0, 0]
    assert float((out - t64([50.0 - 50.0 * 0.5 / 4.0, 50.0 - 50.0 * 1.0 / 4.0]) / n).abs().max()) <= 1e-15
    # far outside the image: clamped at both ends
    out = ref.project_joints_to_views(t64([[[10.0, -10.0, 0.0]]]), R, T, fov, S, None)[0, 0, 0]
    assert out.tolist() == [1.0, 0.0]


def test_regular_sets_are_regular():
    for (B, V, J) in ((2, 2, 3), (65, 7, 65), (257, 2, 3)):
        c = cases.regular(B, V, J, seed=B)
        cases.check_regular(c, 2.0 - 1e-9)
        share_out, share_inv = float(c["outside"].double().mean()), 1.0 - float(c["visibility"].double().mean())
        if B * V * J >= 1000:
            assert abs(share_out - cases.OUTSIDE_SHARE) < 0.03 and abs(share_inv - cases.INVISIBLE_SHARE) < 0.03
        # the cameras are rotations looking at the origin: the origin projects to the centre
        eye = c["R"] @ c["R"].transpose(-1, -2)
        assert float((eye - torch.eye(3, dtype=F64)).abs().max()) <= 1e-12
        centre = ref.project_joints_to_views(torch.zeros(B, 1, 3, dtype=F64), c["R"], c["T"], c["fov"], c["S"], c["aspect"])
        assert float((centre - 0.5).abs().max()) <= 1e-9
    wide = cases.regular(65, 7, 65, seed=3, radius=2.0)
    cases.check_regular(wide, 1.0 - 1e-9)
    yx, _ = ref.project_unclamped(wide["joints"], wide["R"], wide["T"], wide["fov"], wide["S"], wide["aspect"])
    assert bool((yx < 0).any()) and bool((yx > 1).any())


def test_triangulating_noise_free_projections_returns_the_joints():
    for (B, V, J) in ((2, 2, 3), (65, 7, 65), (64, 3, 64)):
        c = cases.regular(B, V, J, seed=7 + V)
        # (the observations are the projections before the clamp: exact, whether or not they fall inside the image)
        M, _, _ = ref.dlt_system(c["observed"], None, c["R"], c["T"], c["fov"], c["S"], c["aspect"])
        cond = torch.linalg.cond(M)
        assert float(cond.max()) <= 1e3, float(cond.max())
        p, valid = ref.triangulate_joints_dlt(c["observed"], None, c["R"], c["T"], c["fov"], c["S"], c["aspect"])
        assert bool(valid.all())
        # the divisor S + 1e-8 against S (an error of 4e-11 relative in the observations) and the damping 1e-6 against M >= 1 move
        # the solution by about 1e-6 |p|
        assert float((p - c["joints"]).abs().max()) <= 1e-5
        loss = ref.triangulation_consistency_loss(c["observed"], None, c["joints"], c["R"], c["T"], c["fov"], c["S"], c["aspect"])
        assert float(loss) <= 1e-10
    # with the regular visibility every joint seen twice or more keeps the bound
    c = cases.regular(65, 7, 65, seed=1)
    M, _, seen = ref.dlt_system(c["observed"], c["visibility"], c["R"], c["T"], c["fov"], c["S"], c["aspect"])
    twice = seen.sum(1) >= 2
    assert float(torch.linalg.cond(M)[twice].max()) <= 1e3


# ---- the public module's checks --------------------------------------------------------------------------------------------------
def test_argument_validation_before_any_device():
    from smilify_amd import keypoint_losses as kl

    c = cases.regular(2, 3, 4)
    j, R, T, fov, tgt, vis, S = c["joints"], c["R"], c["T"], c["fov"], c["target"], c["visibility"], c["S"]
    with pytest.raises(ValueError, match="reduction"):
        kl.keypoint_loss_2d(c["proj"], tgt, vis, reduction="mean")
    with pytest.raises(ValueError, match="reduction"):
        kl.keypoint_loss_3d(j, j, None, reduction="samples")
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(j, j, None)  # trailing size 3
    with pytest.raises(ValueError):
        kl.keypoint_loss_3d(c["proj"], c["proj"], None)  # trailing size 2
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"], tgt[:, :2], vis)
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"], tgt, vis[..., :3])
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"], tgt, vis, mask=torch.ones(2))
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"], tgt, vis, joint_weights=torch.ones(5))
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"], tgt.float(), vis)  # mixed storage types
    with pytest.raises(ValueError):
        kl.keypoint_loss_2d(c["proj"].half(), tgt.half(), vis)
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j[..., :2], R, T, fov, S)
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j, R[:1], T, fov, S)  # B differs
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j, R, T[:, :2], fov, S)  # V differs
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j, R.reshape(2, 3, 9), T, fov, S)
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j, R, T, fov, 0)
    with pytest.raises(ValueError):
        kl.project_joints_to_views(j, [R[:, 0], R[:, 1]], [T[:, 0]], [fov[:, 0], fov[:, 1]], S)
    with pytest.raises(ValueError):
        kl.multiview_keypoint_loss(j, R, T, fov, tgt[:, :, :3], vis, S)  # J differs
    with pytest.raises(ValueError):
        kl.multiview_keypoint_loss(j, R, T, fov, tgt, vis, S, view_mask=torch.ones(2, 4))
    with pytest.raises(ValueError):
        kl.triangulate_joints_dlt(tgt[:, :2], vis[:, :2], R, T, fov, S)  # V differs
    with pytest.raises(ValueError):
        kl.triangulate_joints_dlt(tgt, vis, R, T, fov, S, damping=-1.0)
    with pytest.raises(ValueError, match="damping"):
        kl.triangulate_joints_dlt(tgt, vis, R, T, fov, S, damping=0.0)  # a joint seen by fewer than two views would be singular
    with pytest.raises(ValueError, match="damping"):
        kl.triangulation_consistency_loss(tgt, vis, j, R, T, fov, S, damping=0.0)
    with pytest.raises(ValueError):
        kl.triangulation_consistency_loss(tgt, vis, j[:, :3], R, T, fov, S)


def test_a_cpu_tensor_raises():
    from smilify_amd import keypoint_losses as kl
    from smilify_amd._lib import SmilError

    c = cases.regular(2, 3, 4)
    j, R, T, fov, tgt, vis, S = c["joints"], c["R"], c["T"], c["fov"], c["target"], c["visibility"], c["S"]
    for call in (lambda: kl.keypoint_loss_2d(c["proj"], tgt, vis), lambda: kl.keypoint_loss_3d(j, j, None),
                 lambda: kl.project_joints_to_views(j, R, T, fov, S), lambda: kl.multiview_keypoint_loss(j, R, T, fov, tgt, vis, S),
                 lambda: kl.triangulate_joints_dlt(tgt, vis, R, T, fov, S),
                 lambda: kl.triangulation_consistency_loss(tgt, vis, j, R, T, fov, S)):
        with pytest.raises(SmilError):
            call()


def test_library_rejects_bad_arguments_without_a_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    assert lib.smil_kp_se_forward(None, None, None, None, None, -1, 3, 2, 0, 0, 0, None, None, None, None) == -1
    assert lib.smil_kp_se_forward(None, None, None, None, None, 0, 3, 4, 0, 0, 0, None, None, None, None) == -1 and b"D=4" in lib.smil_last_error()
    assert lib.smil_kp_se_forward(None, None, None, None, None, 0, 3, 2, 0, 7, 0, None, None, None, None) == -1
    assert lib.smil_kp_se_backward(None, None, None, None, None, None, None, None, 0, 3, 2, 16, 0, None) == -1
    assert lib.smil_kp_project(None, None, None, None, None, 1, 1, 1, 0.0, 0, None, None) == -1
    assert lib.smil_kp_project(None, None, None, None, None, 1, 1, 1, 8.0, 2, None, None) == -1 and b"dtype" in lib.smil_last_error()
    assert lib.smil_kp_project(None, None, None, None, None, 0, 1, 1, 8.0, 0, None, None) == 0  # empty: nothing to do
    assert lib.smil_kp_triangulate(None, None, None, None, None, None, None, 1, 1, 1, 8.0, -1.0, 0.0, 0, None, None, None, None) == -1
    assert lib.smil_kp_triangulate(None, None, None, None, None, None, None, 1, 1, 1, 8.0, 0.0, 0.0, 0, None, None, None, None) == -1
    assert b"damping" in lib.smil_last_error()
    assert lib.smil_kp_triangulate_backward(None, None, None, None, None, None, None, None, 1, 1, 1, 8.0, 0.0, 0, None, None, None, None, None) == -1
