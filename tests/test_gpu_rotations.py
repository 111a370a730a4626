"""The rotation kernels (smilify_amd/csrc/rotations.hip, smilify_amd.rotations) against the float64 restatement tests/rotations_ref.py
on the same input values (a float32 input is upcast exactly), values and first-order gradients.

The bounds are derived, not measured (the kernels evaluate in float64 whatever the storage type), per row of one rotation, with S the
largest |ref| of the row:

* float32 storage: ``|got - ref| <= 1.2e-7 |ref| + 1e-10 S``.  Rounding to float32 contributes 2^-24 |ref| = 6e-8 |ref|, the bound is
  twice that; the float64 evaluation contributes below 1e-10 S.
* float64 storage: ``|got - ref| <= 1e-10 max(1, S)``: about 100 operations at 2^-53 with condition numbers up to 1e4 on the stated
  sets.  On degenerate 6-D rows, whose gradients are of order 1e12, the same bound relative to S.
"""
import math

import pytest
import torch

import rotations_cases as cases
import rotations_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
SIZES = [0, 1, 63, 64, 65, 257]
ONE_PASS = 2048 * 256  # rotations one pass of the capped grid covers (ROT_MAX_BLOCKS x ROT_THREADS, csrc/rotations.hip)


def _rotations():
    from smilify_amd import rotations

    return rotations


def close(got, want, dtype, what, relative=False):
    """Assert the module's bound per row (the leading axis of ``want``); prints the worst error over the bound first."""
    want = want.detach().cpu().double()
    rows = want.shape[0]
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if rows == 0:
        return
    got, want = got.detach().cpu().double().reshape(rows, -1), want.reshape(rows, -1)
    S = want.abs().amax(dim=1, keepdim=True)
    if dtype == torch.float32:
        bound = 1.2e-7 * want.abs() + 1e-10 * S
    else:
        bound = (1e-10 * (S if relative else S.clamp(min=1.0))).expand_as(want)
    err = (got - want).abs()
    over = err > bound
    worst = float((err / bound.clamp(min=1e-300)).max()) if bool((bound > 0).any()) else 0.0
    print(f"{what} [{str(dtype)[6:]}]: max err {float(err.max()):.3g}, worst err / bound {worst:.3g}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    assert not bool(over.any()), f"{what}: {int(over.sum())} elements over the bound, worst err / bound {worst:.3g}"


# name -> (public function, reference, which input of a case set, trailing shape of one input, values of one output)
def conversions():
    r = _rotations()
    return {
        "rot6d_to_matrix": (r.rotation_6d_to_matrix, ref.rotation_6d_to_matrix, "d6", (6,), 9),
        "axis_angle_to_matrix": (r.axis_angle_to_matrix, ref.axis_angle_to_matrix, "aa", (3,), 9),
        "matrix_to_axis_angle": (r.matrix_to_axis_angle, ref.matrix_to_axis_angle, "R", (3, 3), 3),
        "rot6d_to_axis_angle": (r.rotation_6d_to_axis_angle, ref.rotation_6d_to_axis_angle, "d6", (6,), 3),
    }


NAMES = ["rot6d_to_matrix", "axis_angle_to_matrix", "matrix_to_axis_angle", "rot6d_to_axis_angle"]


def run(name, x_cpu, dtype, what, relative=False, seed=11):
    """One conversion on the GPU, values and the gradient of sum(out * w), against the reference at the same (cast) input values.
    Returns (out, gradient on the input)."""
    fn, ref_fn, _, tail, k_out = conversions()[name]
    x = x_cpu.to(dtype).to(DEV).clone().requires_grad_(True)
    out = fn(x)
    assert out.dtype == dtype and out.device == x.device
    w = cases.weights(tuple(out.shape), seed).to(dtype)
    (out * w.to(DEV)).sum().backward()
    want, (want_g,) = ref.value_and_grads(ref_fn, [x], w)
    k_in = math.prod(tail)
    n = x.numel() // k_in  # one row per rotation
    close(out.reshape(n, k_out), want.reshape(n, k_out), dtype, f"{what} {name} value", relative)
    close(x.grad.reshape(n, k_in), want_g.reshape(n, k_in), dtype, f"{what} {name} gradient", relative)
    return out.detach(), x.grad.detach()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_regular_set(name, n, dtype):
    c = cases.regular(n)
    key = conversions()[name][2]
    x = c[key].to(dtype)
    if n:
        cases.check_regular(**{key: x})
    run(name, x, dtype, f"regular n={n}")


@pytest.mark.parametrize("name", NAMES)
def test_stride_loop_runs_past_one_pass_of_the_grid(name):
    n = ONE_PASS + 1
    x = cases.regular(n)[conversions()[name][2]].float()
    cases.check_regular(**{conversions()[name][2]: x})
    run(name, x, torch.float32, f"n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_leading_shape_and_non_contiguous_input(name, dtype):
    _, _, key, tail, _ = conversions()[name]
    x = cases.regular(21)[key].to(dtype)
    flat_out, flat_grad = run(name, x, dtype, "flat")
    out, grad = run(name, x.reshape((3, 7) + tail), dtype, "(3,7,.)")
    assert out.shape[:2] == (3, 7) and torch.equal(out.reshape(flat_out.shape), flat_out) and torch.equal(grad.reshape(flat_grad.shape), flat_grad)
    # the same values as every other row of a wider tensor (and, for matrices, as a transposed view)
    fn = conversions()[name][0]
    wide = torch.stack([x, x + 1.0], dim=1).to(DEV)
    view = wide[:, 0]
    assert not view.is_contiguous()
    assert torch.equal(fn(view), flat_out)
    if key == "R":
        xt = x.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)
        assert not xt.is_contiguous() and torch.equal(fn(xt), flat_out)
    leaf = wide.clone().requires_grad_(True)
    out = fn(leaf[:, 0])
    (out * cases.weights(tuple(out.shape), 11).to(dtype).to(DEV)).sum().backward()
    assert torch.equal(leaf.grad[:, 0], flat_grad) and not bool(leaf.grad[:, 1].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_small_angle_set(dtype):
    s = cases.small_angle()
    run("axis_angle_to_matrix", s["aa"], dtype, "small angles")
    run("matrix_to_axis_angle", s["R"], dtype, "small angles")
    # the edge facts, on the device: d aa_x / d m21 = 1/2 at I, d R21 / d a_x = 1 at 0
    r = _rotations()
    m = torch.eye(3, dtype=dtype, device=DEV).requires_grad_(True)
    aa = r.matrix_to_axis_angle(m)
    aa[0].backward()
    assert torch.equal(aa.detach().cpu(), torch.zeros(3, dtype=dtype))
    assert float(m.grad[2, 1]) == 0.5 and float(m.grad[1, 2]) == -0.5 and float(m.grad.abs().sum()) == 1.0
    a = torch.zeros(3, dtype=dtype, device=DEV, requires_grad=True)
    R = r.axis_angle_to_matrix(a)
    R[2, 1].backward()
    assert torch.equal(R.detach().cpu(), torch.eye(3, dtype=dtype)) and a.grad.cpu().tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_degenerate_6d_rows(dtype):
    d = cases.degenerate_6d()
    out, grad = run("rot6d_to_matrix", d, dtype, "degenerate", relative=True)
    assert torch.equal(out[0].cpu(), torch.zeros(3, 3, dtype=dtype))
    assert torch.equal(out[1, 1:].cpu(), torch.zeros(2, 3, dtype=dtype)) and torch.equal(out[7, 1:].cpu(), torch.zeros(2, 3, dtype=dtype))
    if dtype == torch.float64:  # (the float32 nearest 1e-13 is another number)
        assert out[3, 0].cpu().tolist() == [0.1, 0.0, 0.0]
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 1e11
    run("rot6d_to_axis_angle", d, dtype, "degenerate", relative=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_half_turn_set_through_rebuilt_matrices(dtype):
    """The axis sign is discontinuous at a half turn: the matrices rebuilt (by the reference) from the returned axis-angle are compared."""
    R = cases.half_turn().to(dtype)
    got = _rotations().matrix_to_axis_angle(R.to(DEV))
    want = ref.matrix_to_axis_angle(R.double())
    assert bool((got.cpu().double().norm(dim=1) <= math.pi + 1e-6).all())
    dR = (ref.axis_angle_to_matrix(got.cpu().double()) - ref.axis_angle_to_matrix(want)).abs().max()
    print(f"half turn [{str(dtype)[6:]}]: |dR| {float(dR):.3g}")
    assert float(dR) <= (1e-6 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_fused_6d_to_axis_angle_equals_the_two_step_path(dtype):
    """Against the reference's two-step path with the module's bounds (``run``), and with float64 storage, where the two-step path's
    matrix in memory is not rounded, against the device's own two steps."""
    r = _rotations()
    x = cases.regular(257)["d6"].to(dtype)
    fused, fused_grad = run("rot6d_to_axis_angle", x, dtype, "fused")
    leaf = x.to(DEV).requires_grad_(True)
    two = r.matrix_to_axis_angle(r.rotation_6d_to_matrix(leaf))
    (two * cases.weights(tuple(two.shape), 11).to(dtype).to(DEV)).sum().backward()
    if dtype == torch.float64:
        close(fused, two, dtype, "fused against two kernels, value")
        close(fused_grad, leaf.grad, dtype, "fused against two kernels, gradient")


def _distance(p_cpu, t_cpu, dtype, what, need=(True, True)):
    r = _rotations()
    p = p_cpu.to(dtype).to(DEV).clone().requires_grad_(need[0])
    t = t_cpu.to(dtype).to(DEV).clone().requires_grad_(need[1])
    dist = r.rotation_6d_distance(p, t)
    assert dist.shape == p.shape[:-1] and dist.dtype == dtype
    w = cases.weights(tuple(dist.shape), 13).to(dtype)
    (dist * w.to(DEV)).sum().backward()
    want, (gp, gt) = ref.value_and_grads(ref.rotation_6d_distance, [p, t], w)
    close(dist.reshape(-1, 1), want.reshape(-1, 1), dtype, f"{what} distance")
    for x, g, n, side in ((p, gp, need[0], "pred"), (t, gt, need[1], "target")):
        if n:
            close(x.grad.reshape(-1, 6), g.reshape(-1, 6), dtype, f"{what} gradient on {side}")
        else:
            assert x.grad is None
    return dist.detach(), want, p.grad, t.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_distance_regular_pairs(n, dtype):
    p, t, _, _ = cases.distance_pairs(n)
    _distance(p, t, dtype, f"regular pairs n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_distance_gradient_to_either_input_and_leading_shape(dtype):
    p, t, _, _ = cases.distance_pairs(21)
    _, _, gp, gt = _distance(p, t, dtype, "both")
    _, _, gp1, none = _distance(p, t, dtype, "pred only", need=(True, False))
    _, _, none2, gt1 = _distance(p, t, dtype, "target only", need=(False, True))
    assert none is None and none2 is None and torch.equal(gp1, gp) and torch.equal(gt1, gt)
    _, _, gp3, gt3 = _distance(p.reshape(3, 7, 6), t.reshape(3, 7, 6), dtype, "(3,7,6)")
    assert torch.equal(gp3.reshape(21, 6), gp) and torch.equal(gt3.reshape(21, 6), gt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_distance_of_close_and_identical_pairs(dtype):
    _, _, q, near = cases.distance_pairs(257)
    _, want, _, _ = _distance(q, near, dtype, "near pairs")
    assert cases.NEAR_DISTANCE[0] <= float(want.min()) and float(want.max()) <= cases.NEAR_DISTANCE[1]
    dist, _, gp, gt = _distance(q, q.clone(), dtype, "identical pairs")
    assert not bool(dist.any()) and not bool(gp.any()) and not bool(gt.any())  # exactly zero, gradients included


def test_distance_stride_loop():
    n = ONE_PASS + 1
    p, t, _, _ = cases.distance_pairs(n)
    _distance(p.float(), t.float(), torch.float32, f"n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_visibility_weighted_rotation_loss(dtype):
    """Against the reference formula in float64.  The distances carry the module's bound, E below; torch's reduction in the storage
    type adds, with u the type's unit roundoff (2^-24, 2^-53) and n terms that are all >= 0: n - 1 roundings of the sum, one of the
    count plus 1e-8, one of the division and one of the final + 1e-8, so ``|loss - ref| <= (n + 3) u |ref| + E`` with
    E = (1.2e-7 + 1e-10) |ref| for float32 and 1e-10 max(1, 2 sqrt 2) for float64 (no two rotations are further apart than 2 sqrt 2,
    and the loss is an average of distances).  The upstream gradient of a distance is vis / (count + 1e-8), rounded twice (the sum
    and the quotient), so a gradient row is within the module's bound plus ``2 u |ref|``."""
    r = _rotations()
    n = 21
    p_cpu, t_cpu, _, _ = cases.distance_pairs(n)
    f32 = dtype == torch.float32
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    masks = dict(all=torch.ones(3, 7), part=(torch.arange(n) % 3 != 1).float().reshape(3, 7), none=torch.zeros(3, 7))
    for key, vis in masks.items():
        p = p_cpu.to(dtype).reshape(3, 7, 6).to(DEV).requires_grad_(True)
        t = t_cpu.to(dtype).reshape(3, 7, 6).to(DEV)
        loss = r.visibility_weighted_rotation_loss(p, t, vis.to(DEV))
        loss.backward()
        p64 = p.detach().cpu().double().requires_grad_(True)
        want = ref.visibility_weighted_rotation_loss(p64, t.cpu().double(), vis.double())
        if key == "none":
            assert float(loss.detach()) == float(torch.tensor(1e-8, dtype=dtype)) and loss.is_leaf and p.grad is None
            continue
        want.backward()
        got_v, want_v = float(loss.detach()), float(want.detach())
        bound = (n + 3) * u * want_v + ((1.2e-7 + 1e-10) * want_v if f32 else 1e-10 * 2.0 * math.sqrt(2.0))
        print(f"visibility loss {key} [{str(dtype)[6:]}]: {got_v:.17g} vs {want_v:.17g}, err / bound {abs(got_v - want_v) / bound:.3g}")
        assert abs(got_v - want_v) <= bound
        g, g64 = p.grad.cpu().double().reshape(n, 6), p64.grad.reshape(n, 6)
        S = g64.abs().amax(dim=1, keepdim=True)
        kernel = 1.2e-7 * g64.abs() + 1e-10 * S if f32 else 1e-10 * S.clamp(min=1.0)
        assert bool(((g - g64).abs() <= kernel + 2 * u * g64.abs()).all())
        assert not bool(g[vis.reshape(-1) == 0].any())


ENTRY_POINTS = [  # (entry point, widths of its input rows, widths of its output rows)
    ("smil_rot6d_to_matrix", (6,), (9,)), ("smil_rot6d_to_matrix_backward", (6, 9), (6,)),
    ("smil_axis_angle_to_matrix", (3,), (9,)), ("smil_axis_angle_to_matrix_backward", (3, 9), (3,)),
    ("smil_matrix_to_axis_angle", (9,), (3,)), ("smil_matrix_to_axis_angle_backward", (9, 3), (9,)),
    ("smil_rot6d_to_axis_angle", (6,), (3,)), ("smil_rot6d_distance", (6, 6), (1,)), ("smil_rot6d_distance_backward", (6, 6, 1), (6, 6)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=[e[0] for e in ENTRY_POINTS])
def test_nothing_is_written_beyond_n_and_streams_agree(entry, dtype):
    """Every entry point with n of the n + 1 rows its buffers hold: the guard row behind each output keeps its fill, and the same call
    on another stream writes the same bits."""
    from smilify_amd import engine

    name, ins, outs = entry
    n = 65
    c = cases.regular(n + 1)
    src = {6: c["d6"], 3: c["aa"], 9: c["R"].reshape(-1, 9), 1: cases.weights((n + 1, 1), 3)}
    if name.startswith("smil_rot6d_distance"):
        inputs = [c["d6"], cases.regular(n + 1, cases.REGULAR_SEED + 1)["d6"]] + ([src[1]] if len(ins) == 3 else [])
    else:
        inputs = [src[ins[0]]] + [cases.weights((n + 1, k), 3) for k in ins[1:]]
    inputs = [t.to(dtype).contiguous().to(DEV) for t in inputs]
    fill = -777.0

    def call():
        bufs = [torch.full((n + 1, k), fill, dtype=dtype, device=DEV) for k in outs]
        engine.rot_call(name, n, dtype, *inputs, *bufs)
        return bufs

    first = call()
    for b in first:
        assert bool((b[n] == fill).all()), f"{name}: wrote beyond n"
        assert bool(torch.isfinite(b[:n]).all()) and not bool((b[:n] == fill).all(dim=1).any()), f"{name}: a row below n was not written"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = call()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(first, second):
        assert torch.equal(a, b), f"{name}: another stream gave other bits"


def test_6d_output_feeds_smal_with_matrices(tables):
    """Path A: d6 -> rotation_6d_to_matrix -> SMAL(beta, R) -> (verts * probe).sum(), gradient on d6.  Path B: the same SMAL call on
    R.detach() as a leaf, its dR pushed through the float64 reference's vector-Jacobian product at d6.  Float32 bound."""
    from conftest import vertex_probe
    from smilify_amd.smal_torch import SMAL

    r = _rotations()
    t = tables("synthetic")
    smal = SMAL(DEV, tables=t)
    B, J = 3, t.J
    d6_cpu = cases.regular(B * J)["d6"].float().reshape(B, J, 6)
    cases.check_regular(d6=d6_cpu.reshape(-1, 6))
    beta = torch.linspace(-0.5, 0.5, B * t.nB).reshape(B, t.nB).to(DEV)
    probe = vertex_probe((B, t.V, 3), 1).to(DEV)

    d6 = d6_cpu.to(DEV).requires_grad_(True)
    verts = smal(beta, r.rotation_6d_to_matrix(d6))[0]
    (verts * probe).sum().backward()

    R = r.rotation_6d_to_matrix(d6.detach()).requires_grad_(True)
    verts_b = smal(beta, R)[0]
    (verts_b * probe).sum().backward()
    assert torch.equal(verts_b, verts)
    x = d6_cpu.double().requires_grad_(True)
    (want,) = torch.autograd.grad(ref.rotation_6d_to_matrix(x), x, R.grad.cpu().double())
    assert float(want.abs().max()) > 0
    close(d6.grad.reshape(-1, 6), want.reshape(-1, 6), torch.float32, "SMAL gradient on d6")
