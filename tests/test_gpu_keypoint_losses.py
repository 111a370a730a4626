"""The keypoint-loss kernels (smilify_amd/csrc/keypoint_losses.hip, smilify_amd.keypoint_losses) against the float64 restatement
tests/keypoint_losses_ref.py at the same input values (a float32 input is upcast exactly), values and first-order gradients.

The bounds are derived, not measured (the kernels evaluate in float64 whatever the storage type).  They hold per output row - one
projected point (2 values), one joint (3), one camera's R (9), T (3) or fov (1), one loss (1) - with S the row's largest |ref|:

* float64 storage: ``|got - ref| <= 1e-10 max(1, S)``.  A value is about 100 operations at 2^-53 = 1.1e-16 each; the divisions are
  by a view-space depth >= 1 on the stated sets (cases.check_regular), tan is taken at 20 to 30 degrees where it is well conditioned,
  and a sum over J <= 65 joints or V <= 7 views of terms of mixed sign loses at most the terms' magnitude, below 1e3 here, times
  2^-53 per addition: all of it stays under 1e-12 max(1, S), the bound leaves two decades.
* gradients of the triangulation and of the consistency loss: ``1e-8 max(1, S)``.  The backward solves with M twice (p and lambda =
  M^-1 g) and multiplies the two, so cond(M)^2 <= 1e6 (asserted on the set by tests/test_keypoint_losses_cpu.py for joints seen
  twice or more) multiplies the 1e-14 of the arithmetic.  Joints seen by fewer than two views have cond(M) ~ 1e6 and are reported
  invalid: they are checked for finiteness and their flag, and take no upstream gradient here, as in the consistency loss.
* float32 storage: ``1.2e-7 |ref|`` (twice the rounding 2^-24 |ref| of the stored result) plus the float64 bound.

Two device paths compared with each other (fused against two steps, a masked view against the problem without it) are held to the
same bounds, in both storage types: each is a rounding of the same float64 number."""
import pytest
import torch

import keypoint_losses_cases as cases
import keypoint_losses_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
EPS = 1e-8
# (B, V, J): every B of {0, 1, 2, 63, 64, 65, 257}, every J of {1, 3, 64, 65} and every V of {1, 2, 7}; the wave boundary in J with V = 7
SIZES = [(0, 2, 3), (1, 1, 1), (2, 2, 3), (63, 1, 3), (64, 2, 64), (65, 7, 65), (3, 7, 64), (257, 2, 3)]
SIZE_IDS = ["x".join(map(str, s)) for s in SIZES]
ONE_PASS_WAVES = 2048 * 4    # samples one pass of the capped grid covers with a wave each (KP_MAX_BLOCKS x KP_WAVES)
ONE_PASS_THREADS = 2048 * 256  # ... and items with a thread each


def kl():
    from smilify_amd import keypoint_losses

    return keypoint_losses


def close(got, want, dtype, what, width, tol=1e-10):
    """Assert the module's bound per row of ``width`` values; prints the worst error over the bound first."""
    want = want.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == dtype, (what, got.dtype)
    if want.numel() == 0:
        return
    got, want = got.detach().cpu().double().reshape(-1, width), want.reshape(-1, width)
    S = want.abs().amax(dim=1, keepdim=True)
    bound = (tol * S.clamp(min=1.0)).expand_as(want)
    if dtype == torch.float32:
        bound = bound + 1.2e-7 * want.abs()
    err = (got - want).abs()
    worst = float((err / bound).max())
    print(f"{what} [{str(dtype)[6:]}]: max err {float(err.max()):.3g}, worst err / bound {worst:.3g}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    assert not bool((err > bound).any()), f"{what}: {int((err > bound).sum())} elements over the bound, worst err / bound {worst:.3g}"


def cast(c, dtype):
    """The float tensors of a case set rounded to the storage type (still on the CPU: the restatement reads the same values)."""
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}


def dev(x):
    return x.to(DEV) if isinstance(x, torch.Tensor) else x


WIDTH = dict(joints=3, R=9, T=3, fov=1, rendered=2, pred=3)


def compare(gpu_fn, ref_fn, args, wrt, dtype, what, out_width, tol=1e-10, grad_tol=None, up_mask=None, seed=0):
    """``args``: name -> CPU value, in the order both functions take them; ``wrt``: the names that take a gradient.  Compares the
    value and the gradients of sum(value * upstream); returns (value, {name: gradient}) of the device."""
    names = list(args)
    d = {k: dev(v) for k, v in args.items()}
    for k in wrt:
        d[k] = d[k].clone().requires_grad_(True)
    out = gpu_fn(*d.values())
    value = out[0] if isinstance(out, tuple) else out
    up = cases.upstream(value.shape, seed).to(dtype)
    if up_mask is not None:
        up = up * up_mask.to(dtype)
    if wrt:
        (value * dev(up)).sum().backward()
    want_out, want_grads = ref.value_and_grads(ref_fn, list(args.values()), [names.index(k) for k in wrt], up)
    want = want_out[0] if isinstance(want_out, tuple) else want_out
    if up_mask is None:
        close(value, want, dtype, f"{what} value", out_width, tol)
    else:  # rows outside the mask: finite, and not compared
        rows = up_mask.reshape(-1, out_width)[:, 0] != 0
        assert bool(torch.isfinite(value).all())
        close(value.detach().cpu().reshape(-1, out_width)[rows], want.reshape(-1, out_width)[rows], dtype, f"{what} value", out_width, tol)
    grads = {}
    for k, g in zip(wrt, want_grads):
        close(d[k].grad, g, dtype, f"{what} gradient on {k}", WIDTH[k], grad_tol or tol)
        grads[k] = d[k].grad
    return out, grads


REGULAR = {}


def regular(B, V, J, dtype, radius=1.0):
    """A regular set, built once per size and shared (read-only) by the tests that use it."""
    key = (B, V, J, dtype, radius)
    if key not in REGULAR:
        REGULAR[key] = cast(cases.regular(B, V, J, seed=B + V + J, radius=radius), dtype)
    return REGULAR[key]


# ---- (a) the squared-error family --------------------------------------------------------------------------------------------------
def loss_2d_args(c, weights=None, mask=None):
    return dict(rendered=c["proj"], target=c["target"], visibility=c["visibility"], joint_weights=weights, mask=mask)


def gpu_2d(reduction):
    return lambda r, t, v, w, m: kl().keypoint_loss_2d(r, t, v, joint_weights=w, mask=m, reduction=reduction)


def ref_2d(reduction):
    return lambda r, t, v, w, m: ref.keypoint_loss_2d(r, t, v, w, m, reduction)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_loss_2d_sizes_and_reductions(size, dtype):
    B, V, J = size
    c = regular(B, V, J, dtype)
    cases.check_regular(c, 2.0 - 1e-6)
    w = cases.joint_weights(J)
    gen = torch.Generator().manual_seed(5)
    mask = torch.rand(B, V, generator=gen) < 0.7
    for reduction in ("pooled", "valid_samples", "samples"):
        for weights, m in ((None, None), (w, mask)):
            compare(gpu_2d(reduction), ref_2d(reduction), loss_2d_args(c, weights, m), ["rendered"], dtype,
                    f"2-D {reduction} {size} weights={weights is not None}", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loss_3d_reductions_and_rules(dtype):
    """Sentinel rows, non-finite targets and non-finite predictions are not valid; the rest is compared."""
    pred, target, vis = cases.points_3d(65, 65)
    target[0, :3] = 0.0                     # the all-zero sentinel
    target[1, 0, 1] = float("inf")
    target[1, 1, 2] = float("nan")
    pred[2, 5, 0] = float("nan")
    pred[2, 6, 1] = float("-inf")
    target[3] = 0.0                         # a sample of sentinels only: no valid joint
    vis[4] = False                          # and an invisible one
    pred, target = pred.to(dtype), target.to(dtype)
    w = cases.joint_weights(65)
    for reduction in ("valid_samples", "pooled"):
        for weights in (None, w):
            args = dict(pred=pred, target=target, visibility=vis, joint_weights=weights)
            _, g = compare(lambda p, t, v, ww: kl().keypoint_loss_3d(p, t, v, joint_weights=ww, reduction=reduction),
                           lambda p, t, v, ww: ref.keypoint_loss_3d(p, t, v, ww, None, reduction), args, ["pred"], dtype, f"3-D {reduction}", 1)
            g = g["pred"].cpu()
            assert not bool(g[0, :3].any()) and not bool(g[1, :2].any()) and not bool(g[2, 5:7].any()) and not bool(g[3].any()) and not bool(g[4].any())
            assert bool(g[0, 3:].any()) and bool(g[5].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", [(0, 3), (1, 1), (2, 3), (63, 64), (64, 65), (65, 3), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_3d_sizes(size, dtype):
    """N itself at every value of the list (the 2-D tests run N = B V), with and without weights, both reductions."""
    N, J = size
    pred, target, vis = cases.points_3d(N, J, seed=N)
    if N > 1:
        target[1] = 0.0  # a sample of sentinels among valid ones
    for reduction, weights in (("valid_samples", None), ("pooled", cases.joint_weights(J))):
        args = dict(pred=pred.to(dtype), target=target.to(dtype), visibility=vis, joint_weights=weights)
        compare(lambda p, t, v, ww: kl().keypoint_loss_3d(p, t, v, joint_weights=ww, reduction=reduction),
                lambda p, t, v, ww: ref.keypoint_loss_3d(p, t, v, ww, None, reduction), args, ["pred"], dtype, f"3-D {size} {reduction}", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loss_sample_without_a_valid_joint_changes_the_valid_samples_mean(dtype):
    c = dict(regular(65, 2, 3, dtype))
    vis = c["visibility"].clone()
    vis[3, 1] = False
    vis[7] = False
    c["visibility"] = vis
    values = {}
    for reduction in ("valid_samples", "samples", "pooled"):
        out, g = compare(gpu_2d(reduction), ref_2d(reduction), loss_2d_args(c), ["rendered"], dtype, f"empty samples, {reduction}", 1)
        values[reduction] = float(out.detach())
        assert not bool(g["rendered"][3, 1].any()) and not bool(g["rendered"][7].any())
    assert values["valid_samples"] > values["samples"]  # the same sum over fewer samples


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loss_masks_of_every_type_agree(dtype):
    c = regular(64, 2, 64, dtype)
    gen = torch.Generator().manual_seed(9)
    mask = torch.rand(64, 2, generator=gen) < 0.6
    results = []
    for conv in (lambda m: m, lambda m: m.to(torch.uint8), lambda m: m.float() * 2.5, lambda m: m.to(torch.int64) * -3, lambda m: m.double()):
        r = dev(c["proj"]).clone().requires_grad_(True)
        loss = kl().keypoint_loss_2d(r, dev(c["target"]), dev(conv(c["visibility"])), mask=dev(conv(mask)), reduction="valid_samples")
        loss.backward()
        results.append((loss.detach(), r.grad))
    for loss, g in results[1:]:
        assert torch.equal(loss, results[0][0]) and torch.equal(g, results[0][1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loss_everything_masked_is_exactly_eps(dtype):
    c = regular(65, 7, 65, dtype)
    eps = float(torch.tensor(EPS, dtype=torch.float64).to(dtype))
    for reduction in ("pooled", "valid_samples", "samples"):
        for kw in (dict(visibility=torch.zeros(65, 7, 65)), dict(visibility=c["visibility"], mask=torch.zeros(65, 7))):
            r = dev(c["proj"]).clone().requires_grad_(True)
            loss = kl().keypoint_loss_2d(r, dev(c["target"]), dev(kw["visibility"]), mask=dev(kw.get("mask")), reduction=reduction)
            loss.backward()
            assert float(loss.detach()) == eps, (reduction, float(loss.detach()))
            assert not bool(r.grad.any()) and bool(torch.isfinite(r.grad).all())
    pred, target, _ = cases.points_3d(3, 5)
    p = dev(pred.to(dtype)).clone().requires_grad_(True)
    loss = kl().keypoint_loss_3d(p, dev(torch.zeros_like(target).to(dtype)), None)
    loss.backward()
    assert float(loss.detach()) == eps and not bool(p.grad.any())
    # all-zero weights: 0 / (0 + eps) + eps
    r = dev(c["proj"]).clone().requires_grad_(True)
    loss = kl().keypoint_loss_2d(r, dev(c["target"]), dev(c["visibility"]), joint_weights=dev(torch.zeros(65)))
    loss.backward()
    assert float(loss.detach()) == eps and not bool(r.grad.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loss_2d_boundary_rules(dtype):
    """Targets exactly 0 and 1 are in bounds, their neighbours outside are not; predictions exactly 0 and 1 take a gradient; NaN and
    +-inf predictions count as 0, take none and leave the other entries alone."""
    one, zero = torch.tensor(1.0, dtype=dtype), torch.tensor(0.0, dtype=dtype)
    above, below = torch.nextafter(one, torch.tensor(2.0, dtype=dtype)), torch.nextafter(zero, torch.tensor(-1.0, dtype=dtype))
    target = torch.tensor([[[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [0.5, 0.5], [0.25, 0.75], [0.25, 0.75], [0.25, 0.75], [0.3, 0.6]]], dtype=dtype)
    target[0, 2, 0], target[0, 3, 1] = above, below
    rendered = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [0.1, 0.1], [0.1, 0.1], [float("nan"), 0.5], [0.5, float("inf")], [float("-inf"), 0.5],
                              [0.4, 0.4]]], dtype=dtype)
    vis = torch.ones(1, 8)
    for reduction in ("pooled", "valid_samples", "samples"):
        args = dict(rendered=rendered, target=target, visibility=vis, joint_weights=None, mask=None)
        out, g = compare(gpu_2d(reduction), ref_2d(reduction), args, ["rendered"], dtype, f"boundaries {reduction}", 1)
        g = g["rendered"].cpu()[0]
        assert bool((g[0] != 0).all()) and bool((g[1] != 0).all())  # targets at the bounds count, predictions at the bounds take a gradient
        assert not bool(g[2].any()) and not bool(g[3].any())       # a target one step outside does not
        assert g[4, 0] == 0 and g[5, 1] == 0 and g[6, 0] == 0  # the non-finite coordinates
        assert g[4, 1] != 0 and g[5, 0] != 0 and g[6, 1] != 0 and bool((g[7] != 0).all())  # their neighbours and the other joints
        # the same call with zeros in place of the non-finite coordinates: the same bits, value and the other gradients
        pair = []
        for r in (rendered, torch.where(torch.isfinite(rendered), rendered, torch.zeros_like(rendered))):
            r = dev(r).clone().requires_grad_(True)
            loss = kl().keypoint_loss_2d(r, dev(target), dev(vis), reduction=reduction)
            loss.backward()
            pair.append((loss.detach(), r.grad.cpu()[0]))
        keep = torch.isfinite(rendered)[0]
        assert torch.equal(pair[0][0], pair[1][0]) and torch.equal(pair[0][0], out.detach())
        assert torch.equal(pair[0][1][keep], pair[1][1][keep]) and not bool(pair[0][1][~keep].any())


def test_loss_beyond_one_pass_of_the_capped_grid():
    """N = 8193 samples of 65 joints: the wave-per-sample forward and the thread-per-joint backward both stride past one pass."""
    N, J = ONE_PASS_WAVES + 1, 65
    assert N * J > ONE_PASS_THREADS
    gen = torch.Generator().manual_seed(21)
    target = torch.rand(N, J, 2, generator=gen, dtype=torch.float64).float()
    rendered = (target.double() + 0.02 * torch.randn(N, J, 2, generator=gen, dtype=torch.float64)).float()
    vis = torch.rand(N, J, generator=gen) < 0.8
    for reduction in ("pooled", "valid_samples"):
        args = dict(rendered=rendered, target=target, visibility=vis, joint_weights=None, mask=None)
        compare(gpu_2d(reduction), ref_2d(reduction), args, ["rendered"], torch.float32, f"N={N} {reduction}", 1)


# ---- (b) projection ----------------------------------------------------------------------------------------------------------------
def camera_args(c):
    return dict(joints=c["joints"], R=c["R"], T=c["T"], fov=c["fov"], aspect=c["aspect"])


def gpu_project(S):
    return lambda j, R, T, f, a: kl().project_joints_to_views(j, R, T, f, S, a)


def ref_project(S):
    return lambda j, R, T, f, a: ref.project_joints_to_views(j, R, T, f, S, a)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_project_sizes(size, dtype):
    B, V, J = size
    c = regular(B, V, J, dtype, radius=2.0)
    cases.check_regular(c, 1.0 - 1e-6)
    compare(gpu_project(c["S"]), ref_project(c["S"]), camera_args(c), ["joints", "R", "T", "fov"], dtype, f"project {size}", 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_project_gradients_alone_and_together_with_both_clamps(dtype):
    c = regular(65, 7, 65, dtype, radius=2.0)
    yx, _ = ref.project_unclamped(c["joints"], c["R"], c["T"], c["fov"], c["S"], c["aspect"])
    assert bool((yx < 0).any()) and bool((yx > 1).any()) and bool(((yx > 0) & (yx < 1)).any())  # clamped at both ends, and not
    out, together = compare(gpu_project(c["S"]), ref_project(c["S"]), camera_args(c), ["joints", "R", "T", "fov"], dtype, "together", 2)
    assert bool((out == 0).any()) and bool((out == 1).any())
    for name in ("joints", "R", "T", "fov"):
        _, alone = compare(gpu_project(c["S"]), ref_project(c["S"]), camera_args(c), [name], dtype, f"{name} alone", 2)
        assert torch.equal(alone[name], together[name])
    # without an aspect ratio
    args = camera_args(c)
    args["aspect"] = None
    compare(gpu_project(c["S"]), ref_project(c["S"]), args, ["joints", "R", "T", "fov"], dtype, "no aspect", 2)


def test_project_agrees_with_the_renderer_float32_path():
    """``Renderer.set_camera_parameters`` + ``forward(joints_only=True)`` (csrc/project.hip, float32), divided by S and clamped, against
    the new kernel on the same float32 inputs: within 32 x 2^-24 - about ten float32 operations of about 1 ulp each on values up to
    S, normalised by S."""
    from smilify_amd.p3d_renderer import Renderer

    B, V, J = 65, 7, 65
    c = regular(B, V, J, torch.float32)
    S = c["S"]
    renderer = Renderer(S, DEV, views=V)
    renderer.set_camera_parameters(dev(c["R"]).reshape(-1, 3, 3), dev(c["T"]).reshape(-1, 3), dev(c["fov"]).reshape(-1), dev(c["aspect"]).reshape(-1))
    joints = dev(c["joints"])
    _, yx = renderer(joints, joints, None, joints_only=True)
    old = (yx.reshape(B, V, J, 2) / S).clamp(0.0, 1.0)
    new = kl().project_joints_to_views(joints, dev(c["R"]), dev(c["T"]), dev(c["fov"]), S, dev(c["aspect"]))
    err = float((old.double() - new.double()).abs().max())
    print(f"renderer path against the float64 kernel: max err {err:.3g} (bound {32 * 2.0 ** -24:.3g})")
    assert err <= 32 * 2.0 ** -24


# ---- (c) the fused loss ------------------------------------------------------------------------------------------------------------
def fused_args(c, weights=None, view_mask=None):
    return dict(joints=c["joints"], R=c["R"], T=c["T"], fov=c["fov"], target=c["target"], visibility=c["visibility"], aspect=c["aspect"],
                view_mask=view_mask, joint_weights=weights)


def gpu_fused(S):
    return lambda j, R, T, f, t, v, a, vm, w: kl().multiview_keypoint_loss(j, R, T, f, t, v, S, aspect_ratio=a, view_mask=vm, joint_weights=w)


def ref_fused(S):
    return lambda j, R, T, f, t, v, a, vm, w: ref.multiview_keypoint_loss(j, R, T, f, t, v, S, a, vm, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_fused_loss_sizes(size, dtype):
    B, V, J = size
    c = regular(B, V, J, dtype, radius=2.0)
    gen = torch.Generator().manual_seed(6)
    vm = torch.rand(B, V, generator=gen) < 0.8
    for weights, mask in ((None, None), (cases.joint_weights(J), vm)):
        compare(gpu_fused(c["S"]), ref_fused(c["S"]), fused_args(c, weights, mask), ["joints", "R", "T", "fov"], dtype, f"fused {size}", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_loss_equals_the_two_step_path_and_repeats_its_bits(dtype):
    """Fused against ``keypoint_loss_2d(project_joints_to_views(...), reduction="pooled")`` on the device: value and all four gradients
    agree within the module's bounds in both storage types.  In float32 the two-step path rounds the projected array p to float32
    between its kernels; with |p| <= 1 that moves p - t by at most 2^-24 = 6e-8, the loss (a mean of (p - t)^2 over about 2e4
    terms, p - t ~ 0.02) by about 1e-9 of itself and a gradient row (at most 65 terms of order 1e-6 each) by about 1e-12 absolute,
    far inside ``1.2e-7 |ref| + 1e-10``."""
    c = regular(65, 7, 65, dtype, radius=2.0)
    S, w = c["S"], cases.joint_weights(65)
    gen = torch.Generator().manual_seed(6)
    vm = torch.rand(65, 7, generator=gen) < 0.8
    names = ("joints", "R", "T", "fov")

    def run(fused):
        leaves = {k: dev(c[k]).clone().requires_grad_(True) for k in names}
        if fused:
            loss = kl().multiview_keypoint_loss(leaves["joints"], leaves["R"], leaves["T"], leaves["fov"], dev(c["target"]), dev(c["visibility"]), S,
                                                aspect_ratio=dev(c["aspect"]), view_mask=dev(vm), joint_weights=dev(w))
        else:
            proj = kl().project_joints_to_views(leaves["joints"], leaves["R"], leaves["T"], leaves["fov"], S, dev(c["aspect"]))
            loss = kl().keypoint_loss_2d(proj, dev(c["target"]), dev(c["visibility"]), joint_weights=dev(w), mask=dev(vm), reduction="pooled")
        loss.backward()
        return loss.detach(), {k: v.grad for k, v in leaves.items()}

    loss, grads = run(True)
    again, grads_again = run(True)
    assert torch.equal(loss, again) and all(torch.equal(grads[k], grads_again[k]) for k in names)  # bit-identical, value and gradients
    two, grads_two = run(False)
    close(loss, two, dtype, "fused against two steps, value", 1)
    for k in names:
        close(grads[k], grads_two[k], dtype, f"fused against two steps, gradient on {k}", WIDTH[k])


# ---- (d) triangulation and the consistency loss ----------------------------------------------------------------------------------------
def noisy_observations(c, dtype, seed=0):
    gen = torch.Generator().manual_seed(6000 + seed)
    return (c["observed"].double() + 0.005 * torch.randn(c["observed"].shape, generator=gen, dtype=torch.float64)).to(dtype)


def tri_args(c, kp, view_mask=None):
    return dict(keypoints=kp, visibility=c["visibility"], R=c["R"], T=c["T"], fov=c["fov"], aspect=c["aspect"], view_mask=view_mask)


def gpu_tri(S):
    return lambda kp, v, R, T, f, a, vm: kl().triangulate_joints_dlt(kp, v, R, T, f, S, aspect_ratio=a, view_mask=vm)


def ref_tri(S):
    return lambda kp, v, R, T, f, a, vm: ref.triangulate_joints_dlt(kp, v, R, T, f, S, a, vm)


def cons_args(c, kp, weights=None, view_mask=None):
    return dict(keypoints=kp, visibility=c["visibility"], joints=c["joints"], R=c["R"], T=c["T"], fov=c["fov"], aspect=c["aspect"],
                view_mask=view_mask, joint_weights=weights)


def gpu_cons(S, max_norm=50.0):
    return lambda kp, v, j, R, T, f, a, vm, w: kl().triangulation_consistency_loss(kp, v, j, R, T, f, S, aspect_ratio=a, view_mask=vm,
                                                                                   joint_weights=w, max_norm=max_norm)


def ref_cons(S, max_norm=50.0):
    return lambda kp, v, j, R, T, f, a, vm, w: ref.triangulation_consistency_loss(kp, v, j, R, T, f, S, a, vm, w, max_norm)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_triangulation_and_consistency_sizes(size, dtype):
    B, V, J = size
    c = regular(B, V, J, dtype)
    kp = noisy_observations(c, dtype)
    want_valid = c["visibility"].sum(dim=1) >= 2
    (points, valid), _ = compare(gpu_tri(c["S"]), ref_tri(c["S"]), tri_args(c, kp), ["R", "T", "fov"], dtype, f"triangulate {size}", 3,
                                 grad_tol=1e-8, up_mask=want_valid.unsqueeze(-1).expand(B, J, 3))
    assert valid.dtype == torch.bool and torch.equal(valid.cpu(), want_valid)
    assert bool(torch.isfinite(points).all())  # joints seen by no view or one view included
    for weights in (None, cases.joint_weights(J)):
        compare(gpu_cons(c["S"]), ref_cons(c["S"]), cons_args(c, kp, weights), ["R", "T", "fov"], dtype, f"consistency {size}", 1, grad_tol=1e-8)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_triangulation_of_joints_seen_by_no_view_and_by_one(dtype):
    c = dict(regular(3, 7, 64, dtype))
    kp = noisy_observations(c, dtype)
    vis = c["visibility"].clone()
    vis[:, :, 0] = False      # joint 0: nobody sees it
    vis[:, :, 1] = False
    vis[:, 2, 1] = True       # joint 1: one view
    vis[:, :, 2] = True       # joint 2: everybody
    c["visibility"] = vis
    leaves = {k: dev(c[k]).clone().requires_grad_(True) for k in ("R", "T", "fov")}
    points, valid = kl().triangulate_joints_dlt(dev(kp), dev(vis), leaves["R"], leaves["T"], leaves["fov"], c["S"], aspect_ratio=dev(c["aspect"]))
    assert bool(torch.isfinite(points).all()) and not bool(valid[:, :2].any()) and bool(valid[:, 2].all())
    assert not bool(points[:, 0].any())  # (damping I) p = 0
    # the two joints do not enter the consistency loss or its gradient: moving their keypoints and 3-D targets changes no bit
    def consistency(kp_, joints_):
        for v in leaves.values():
            v.grad = None
        loss = kl().triangulation_consistency_loss(dev(kp_), dev(vis), dev(joints_), leaves["R"], leaves["T"], leaves["fov"], c["S"],
                                                   aspect_ratio=dev(c["aspect"]))
        loss.backward()
        return loss.detach(), [v.grad.clone() for v in leaves.values()]

    loss, grads = consistency(kp, c["joints"])
    kp2, joints2 = kp.clone(), c["joints"].clone()
    kp2[:, :, :2] += 0.125
    joints2[:, :2] += 1.0
    loss2, grads2 = consistency(kp2, joints2)
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    compare(gpu_cons(c["S"]), ref_cons(c["S"]), cons_args(c, kp), ["R", "T", "fov"], dtype, "consistency with unseen joints", 1, grad_tol=1e-8)
    # nobody sees anything: exactly eps, zero gradients
    loss, grads = None, None
    for v in leaves.values():
        v.grad = None
    loss = kl().triangulation_consistency_loss(dev(kp), dev(torch.zeros_like(vis)), dev(c["joints"]), leaves["R"], leaves["T"], leaves["fov"], c["S"],
                                               aspect_ratio=dev(c["aspect"]))
    loss.backward()
    assert float(loss.detach()) == float(torch.tensor(EPS, dtype=torch.float64).to(dtype))
    assert all(not bool(v.grad.any()) and bool(torch.isfinite(v.grad).all()) for v in leaves.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_masked_view_equals_the_problem_without_it(dtype):
    c = regular(3, 7, 64, dtype)
    kp = noisy_observations(c, dtype)
    S, drop = c["S"], 4
    keep = [v for v in range(7) if v != drop]
    vm = torch.ones(3, 7, dtype=torch.bool)
    vm[:, drop] = False

    def run(sel, view_mask, fused):
        leaves = {k: dev(c[k][:, sel].contiguous()).requires_grad_(True) for k in ("R", "T", "fov")}
        R, T, fov = leaves["R"], leaves["T"], leaves["fov"]
        kw = dict(aspect_ratio=dev(c["aspect"][:, sel].contiguous()), view_mask=dev(view_mask))
        k2, vis = dev(kp[:, sel].contiguous()), dev(c["visibility"][:, sel].contiguous())
        if fused:
            loss = kl().multiview_keypoint_loss(dev(c["joints"]), R, T, fov, dev(c["target"][:, sel].contiguous()), vis, S, **kw)
            points = valid = None
        else:
            points, valid = kl().triangulate_joints_dlt(k2, vis, R, T, fov, S, **kw)
            loss = kl().triangulation_consistency_loss(k2, vis, dev(c["joints"]), R, T, fov, S, **kw)
        loss.backward()
        return points, valid, loss.detach(), {k: v.grad for k, v in leaves.items()}

    # triangulation: a masked view is skipped, so every sum runs over the same terms in the same order - the same bits
    masked, without = run(list(range(7)), vm, False), run(keep, None, False)
    assert torch.equal(masked[0], without[0]) and torch.equal(masked[1], without[1]) and torch.equal(masked[2], without[2])
    for k in ("R", "T", "fov"):
        assert torch.equal(masked[3][k][:, keep], without[3][k]) and not bool(masked[3][k][:, drop].any())
    # the fused loss: the masked view's zero partial sits among the others in the final sum, whose order then differs - two
    # roundings of the same number, which is what the storage bound allows
    masked, without = run(list(range(7)), vm, True), run(keep, None, True)
    close(masked[2], without[2], dtype, "fused, masked view, value", 1)
    for k in ("R", "T", "fov"):
        close(masked[3][k][:, keep].contiguous(), without[3][k], dtype, f"fused, masked view, gradient on {k}", WIDTH[k])
        assert not bool(masked[3][k][:, drop].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_consistency_excludes_points_beyond_max_norm(dtype):
    c = regular(65, 7, 65, dtype)
    kp = noisy_observations(c, dtype)
    p, valid = ref.triangulate_joints_dlt(kp, c["visibility"], c["R"], c["T"], c["fov"], c["S"], c["aspect"])
    norm, max_norm = p.norm(dim=-1)[valid], 0.75
    assert bool((norm < max_norm).any()) and bool((norm >= max_norm).any()) and float((norm - max_norm).abs().min()) > 1e-9
    out, _ = compare(gpu_cons(c["S"], max_norm), ref_cons(c["S"], max_norm), cons_args(c, kp, cases.joint_weights(65)), ["R", "T", "fov"], dtype,
                     "max_norm 0.75", 1, grad_tol=1e-8)
    full = kl().triangulation_consistency_loss(dev(kp), dev(c["visibility"]), dev(c["joints"]), dev(c["R"]), dev(c["T"]), dev(c["fov"]), c["S"],
                                               aspect_ratio=dev(c["aspect"]), joint_weights=dev(cases.joint_weights(65)))
    assert float(full.detach()) != float(out.detach())


# ---- argument forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_non_contiguous_inputs_and_per_view_lists_give_the_stacked_results(dtype):
    """Every function once per form of its arguments, each with leaves of its own (one gradient contribution per leaf, so nothing
    depends on the order autograd adds contributions in): the same bits."""
    B, V, J = 3, 7, 64
    c = regular(B, V, J, dtype)
    kp = noisy_observations(c, dtype)
    S = c["S"]
    up = cases.upstream((B, V, J, 2)).to(dtype)
    names = ("joints", "R", "T", "fov")

    def strided(x):
        """the same values as every other element along a new last axis"""
        view = torch.stack([x, x + 1], dim=-1).to(DEV)[..., 0]
        assert not view.is_contiguous()
        return view

    def stacked_form(make):
        leaves = {k: make(c[k]).detach().requires_grad_(True) for k in names}
        return leaves, (leaves["R"], leaves["T"], leaves["fov"]), make(c["aspect"])

    def list_form(_make):
        leaves = {k: dev(c[k]).clone().requires_grad_(True) for k in names}
        R, T, fov = leaves["R"], leaves["T"], leaves["fov"]  # the reference's lists: (B,3,3), (B,3), (B,1) and (B,) per view
        cams = ([R[:, v] for v in range(V)], [T[:, v] for v in range(V)], [fov[:, v:v + 1] for v in range(V)])
        return leaves, cams, [dev(c["aspect"])[:, v] for v in range(V)]

    def run(form, make):
        target, vis, k2 = make(c["target"]), make(c["visibility"].to(dtype)), make(kp)
        results = []
        for which in ("project", "two steps", "fused", "triangulate", "consistency"):
            leaves, cams, aspect = form(make)
            if which == "project":
                out = kl().project_joints_to_views(leaves["joints"], *cams, S, aspect)
                scalar = (out * dev(up)).sum()
            elif which == "two steps":
                out = kl().keypoint_loss_2d(kl().project_joints_to_views(leaves["joints"], *cams, S, aspect), target, vis, reduction="valid_samples")
                scalar = out
            elif which == "fused":
                scalar = out = kl().multiview_keypoint_loss(leaves["joints"], *cams, target, vis, S, aspect_ratio=aspect)
            elif which == "triangulate":
                out, valid = kl().triangulate_joints_dlt(k2, vis, *cams, S, aspect_ratio=aspect)
                scalar = (out * valid.unsqueeze(-1) * dev(up[:, 0, :, :1])).sum()
            else:
                scalar = out = kl().triangulation_consistency_loss(k2, vis, leaves["joints"], *cams, S, aspect_ratio=aspect)
            scalar.backward()
            results.append((which, out.detach(), [leaves[k].grad for k in names]))
        return results

    base = run(stacked_form, lambda x: dev(x).clone())
    for label, other in (("strided", run(stacked_form, strided)), ("lists", run(list_form, lambda x: dev(x).clone()))):
        for (which, out, grads), (_, out2, grads2) in zip(base, other):
            assert torch.equal(out, out2), (label, which)
            for k, a, b in zip(names, grads, grads2):
                assert (a is None and b is None) or torch.equal(a, b), (label, which, k)


def test_visibility_masks_and_weights_on_the_cpu_raise():
    """Nothing is copied to the device behind the caller's back (a pageable copy would block the host)."""
    from smilify_amd._lib import SmilError

    c = regular(2, 2, 3, torch.float32)
    j, R, T, fov, tgt, proj, S = (dev(c[k]) for k in ("joints", "R", "T", "fov", "target", "proj", "S"))
    vis, w, vm = c["visibility"], cases.joint_weights(3), torch.ones(2, 2)
    for call in (lambda: kl().keypoint_loss_2d(proj, tgt, vis), lambda: kl().keypoint_loss_2d(proj, tgt, dev(vis), mask=vm),
                 lambda: kl().keypoint_loss_2d(proj, tgt, dev(vis), joint_weights=w), lambda: kl().keypoint_loss_3d(j, j, vis[:, 0]),
                 lambda: kl().multiview_keypoint_loss(j, R, T, fov, tgt, vis, S), lambda: kl().multiview_keypoint_loss(j, R, T, fov, tgt, dev(vis), S, view_mask=vm),
                 lambda: kl().triangulate_joints_dlt(tgt, vis, R, T, fov, S), lambda: kl().triangulation_consistency_loss(tgt, dev(vis), j, R, T, fov, S, joint_weights=w)):
        with pytest.raises(SmilError):
            call()
