"""The alignment kernels (smilify_amd/csrc/align.hip, smilify_amd.align) against the float64 restatement tests/align_ref.py - Kabsch /
Umeyama through an SVD with autograd, a different algorithm - on the same input values (a float32 input is upcast exactly), values and
first-order gradients, per problem.

Bounds, per problem and quantity (R, t, s, gap, rms, the gradient on src, the gradient on dst), S the largest |ref| of that row:

* float64 storage: values ``1e-10 max(1, S)``, gradients ``1e-9 max(1, S)``.  On the regular set (gap >= 0.01, the cloud at most 1e3
  spreads from the origin) two float64 algorithms agree within 2e-13 on values and 6e-13 / gap on gradients: the bounds leave room.
  t is a row of its own, so it is compared relative to max(1, |t|).
* float32 storage: the float64 bound plus ``1.2e-7 |ref|`` - the kernels compute in float64 and round once, 2^-24 |ref|, and the
  bound is twice that (the rule of tests/test_gpu_rotations.py).

Status, the fall-back outputs and the all-zero gradients of problems that determine no rotation are compared exactly.
"""
import functools

import pytest
import torch

import align_cases as cases
import align_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
BATCHES = [0, 1, 3, 65]
JOINTS = [0, 1, 2, 3, 4, 63, 64, 65, 130]  # the wave edges: one wave holds a problem, lane l takes joints l, l + 64, ...
WORST = {"value": 0.0, "gradient": 0.0}


def _align():
    from smilify_amd import align

    return align


def close(got, want, dtype, what, grad=False, factor=None):
    """Assert the module's bound per problem (the leading axis of ``want``); prints the worst error over the bound first."""
    want = want.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == dtype, (what, got.dtype)
    rows = want.shape[0]
    if want.numel() == 0:
        return
    got, want = got.detach().cpu().double().reshape(rows, -1), want.reshape(rows, -1)
    S = want.abs().amax(dim=1, keepdim=True)
    bound = ((factor or (1e-9 if grad else 1e-10)) * S.clamp(min=1.0)).expand_as(want)
    if dtype == torch.float32:
        bound = bound + 1.2e-7 * want.abs()
    err = (got - want).abs()
    worst = float((err / bound).max())
    key = "gradient" if grad else "value"
    WORST[key] = max(WORST[key], worst)
    print(f"{what} [{str(dtype)[6:]}]: max err {float(err.max()):.3g}, worst err / bound {worst:.3g} (so far: values {WORST['value']:.3g}, "
          f"gradients {WORST['gradient']:.3g})")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    assert not bool((err > bound).any()), f"{what}: {int((err > bound).sum())} elements over the bound, worst err / bound {worst:.3g}"


def upcast(c, dtype):
    """The case as the restatement gets it: the points rounded to ``dtype`` and upcast exactly."""
    return dict(src=c["src"].to(dtype).double(), dst=c["dst"].to(dtype).double(), weights=c["weights"], mask=c["mask"])


def probes(B, seed, dtype):
    """The seeded probe weights as both sides use them: rounded to ``dtype``, float64 (the GPU side casts them back, exactly)."""
    return {k: v.to(dtype).double() for k, v in cases.probes(B, seed).items()}


def cast(c, dtype):
    """(the case as the kernels get it: points in ``dtype`` on the GPU, the same values for the restatement)"""
    dev = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    return dict(src=c["src"].to(dtype).to(DEV), dst=c["dst"].to(dtype).to(DEV), weights=dev(c["weights"]), mask=dev(c["mask"])), upcast(c, dtype)


@functools.lru_cache(maxsize=None)
def reference(B, J, dtype, weights, with_scale):
    """(case, restatement's Transform, its gradients) of the wave-edge set at one shape: computed once, shared, never changed."""
    c = cases.wave_edge(B, J, seed=J + 7 * B, weights=weights)
    cpu = upcast(c, dtype)
    if J >= 4 and B > 0:
        cases.check_regular(**cpu)
    x, _, g = ref.value_and_grads(cpu["src"], cpu["dst"], probes(B, J, dtype), weights=cpu["weights"], mask=cpu["mask"], with_scale=with_scale)
    return c, x, g


def run(gpu, dtype, probes, wrt, **kw):
    """One call on the GPU and the gradients of sum(R pR) + sum(t pt) + sum(s ps) to the inputs named in ``wrt``."""
    leaves = {k: gpu[k].clone().requires_grad_(k in wrt) for k in ("src", "dst")}
    x = _align().similarity_transform(leaves["src"], leaves["dst"], weights=gpu["weights"], mask=gpu["mask"], **kw)
    p = {k: v.to(dtype).to(DEV) for k, v in probes.items()}
    ((x.R * p["R"]).sum() + (x.t * p["t"]).sum() + (x.s * p["s"]).sum()).backward()
    for k in ("src", "dst"):
        assert (leaves[k].grad is not None) == (k in wrt)
    return x, {k: leaves[k].grad for k in wrt}


def check_values(x, want, dtype, what):
    B = want.R.shape[0]
    assert x.status.dtype == torch.int32 and x.status.cpu().tolist() == want.status.tolist(), what
    close(x.R.reshape(B, 9), want.R.reshape(B, 9), dtype, f"{what} R")
    close(x.t, want.t, dtype, f"{what} t")
    for name in ("s", "gap", "rms"):
        close(getattr(x, name).reshape(B, 1), getattr(want, name).reshape(B, 1), dtype, f"{what} {name}")


def check_dead_problems(x, grads, want, what):
    """Problems that are not OK: the identity, s = 1 and all-zero gradients, exactly."""
    dead = (want.status != ref.OK).to(DEV)
    if not bool(dead.any()):
        return
    assert torch.equal(x.R[dead], torch.eye(3, dtype=x.R.dtype, device=DEV).expand(int(dead.sum()), 3, 3)), what
    assert bool((x.s[dead] == 1.0).all()), what
    assert not bool(x.t[(want.status == ref.EMPTY).to(DEV)].any()), what
    for k, g in grads.items():
        assert not bool(g[dead].any()), f"{what}: a gradient on {k} of a problem that determines no rotation"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("J", JOINTS)
@pytest.mark.parametrize("B", BATCHES)
def test_wave_edges_values_and_gradients(B, J, dtype):
    c, want, want_g = reference(B, J, dtype, "BJ", True)
    gpu, _ = cast(c, dtype)
    what = f"B={B} J={J}"
    for wrt in (("src",), ("dst",), ("src", "dst")):
        x, grads = run(gpu, dtype, probes(B, J, dtype), wrt)
        check_values(x, want, dtype, what)
        for k in wrt:
            close(grads[k].reshape(B, 3 * J), want_g[k].reshape(B, 3 * J), dtype, f"{what} gradient on {k} (of {'+'.join(wrt)})", grad=True)
        check_dead_problems(x, grads, want, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("weights,with_scale", [("J", True), (None, True), ("BJ", False), ("J", False)])
def test_weight_layouts_and_the_rigid_solve(weights, with_scale, dtype):
    B, J = 3, 65
    c, want, want_g = reference(B, J, dtype, weights, with_scale)
    gpu, _ = cast(c, dtype)
    x, grads = run(gpu, dtype, probes(B, J, dtype), ("src", "dst"), with_scale=with_scale)
    what = f"weights={weights} with_scale={with_scale}"
    check_values(x, want, dtype, what)
    for k in grads:
        close(grads[k].reshape(B, -1), want_g[k].reshape(B, -1), dtype, f"{what} gradient on {k}", grad=True)
    if not with_scale:
        assert bool((x.s == 1.0).all())
        a = _align()
        y = a.rigid_transform(gpu["src"], gpu["dst"], gpu["weights"], gpu["mask"])
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    # unbatched input: unbatched results, the same bits
    w0 = gpu["weights"] if weights != "BJ" else gpu["weights"][0]
    one = _align().similarity_transform(gpu["src"][0], gpu["dst"][0], weights=w0, mask=gpu["mask"][0], with_scale=with_scale)
    assert tuple(one.R.shape) == (3, 3) and tuple(one.t.shape) == (3,) and one.s.dim() == 0 and one.status.dim() == 0
    assert all(torch.equal(u, v[0]) for u, v in zip(one, x))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_degenerate_sets_are_exact(dtype):
    for name, c, status in cases.degenerate():
        gpu, cpu = cast(c, dtype)
        want, _, _ = ref.value_and_grads(cpu["src"], cpu["dst"], probes(1, 1, dtype), weights=cpu["weights"], mask=cpu["mask"])
        x, grads = run(gpu, dtype, probes(1, 1, dtype), ("src", "dst"))
        assert x.status.cpu().tolist() == [status] == want.status.tolist(), name
        # every sum of these sets is exact, so the fall-back outputs are compared bit for bit
        assert torch.equal(x.R.cpu().double(), want.R) and torch.equal(x.s.cpu().double(), want.s), name
        assert torch.equal(x.t.cpu().double(), want.t.to(dtype).double()), (name, x.t, want.t)
        close(x.gap.reshape(1, 1), want.gap.reshape(1, 1), dtype, f"{name} gap")
        close(x.rms.reshape(1, 1), want.rms.reshape(1, 1), dtype, f"{name} rms")
        assert not bool(grads["src"].any()) and not bool(grads["dst"].any()), name
        assert tuple(grads["src"].shape) == tuple(c["src"].shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_non_finite_coordinates_drop_their_joint(dtype):
    c = cases.with_nan()
    gpu, cpu = cast(c, dtype)
    want, _, want_g = ref.value_and_grads(cpu["src"], cpu["dst"], probes(1, 2, dtype))
    x, grads = run(gpu, dtype, probes(1, 2, dtype), ("src", "dst"))
    check_values(x, want, dtype, "with NaN")
    for k in grads:
        close(grads[k].reshape(1, -1), want_g[k].reshape(1, -1), dtype, f"with NaN gradient on {k}", grad=True)
        assert not bool(grads[k][0, [2, 5]].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_mixed_launch(dtype):
    """Regular and degenerate problems in one batch: every problem answers for itself."""
    c = cases.regular(7, 6, seed=11, weights="BJ", masked=True)
    c["src"][1] = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)  # coincident points
    c["mask"][3] = 0  # nothing left
    c["src"][5] = torch.arange(6, dtype=torch.float64)[:, None] * torch.tensor([0.5, 1.0, -2.0], dtype=torch.float64)  # collinear
    c["mask"][6, 2:] = 0  # two points
    gpu, cpu = cast(c, dtype)
    want, _, want_g = ref.value_and_grads(cpu["src"], cpu["dst"], probes(7, 3, dtype), weights=cpu["weights"], mask=cpu["mask"])
    assert want.status.tolist() == [ref.OK, ref.DEGENERATE, ref.OK, ref.EMPTY, ref.OK, ref.DEGENERATE, ref.DEGENERATE]
    x, grads = run(gpu, dtype, probes(7, 3, dtype), ("src", "dst"))
    check_values(x, want, dtype, "mixed")
    for k in grads:
        close(grads[k].reshape(7, -1), want_g[k].reshape(7, -1), dtype, f"mixed gradient on {k}", grad=True)
    check_dead_problems(x, grads, want, "mixed")


def test_mirrored_targets_get_a_proper_rotation():
    c = cases.regular(65, 12, seed=5)
    gpu, _ = cast(c, torch.float64)
    a = _align()
    for with_scale in (True, False):
        x = a.similarity_transform(gpu["src"], gpu["dst"], gpu["weights"], gpu["mask"], with_scale=with_scale)
        det = torch.linalg.det(x.R.cpu())
        print(f"det R - 1 over 65 problems (13 mirrored), with_scale={with_scale}: {float((det - 1).abs().max()):.3g}")
        assert float((det - 1.0).abs().max()) <= 1e-12
        assert float((x.R @ x.R.transpose(1, 2) - torch.eye(3, dtype=torch.float64, device=DEV)).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_second_call_gives_the_same_bits(dtype):
    c = cases.regular(65, 130, seed=2)
    gpu, _ = cast(c, dtype)
    first = run(gpu, dtype, probes(65, 4, dtype), ("src", "dst"), robust_iters=2, robust_scale=0.5)
    second = run(gpu, dtype, probes(65, 4, dtype), ("src", "dst"), robust_iters=2, robust_scale=0.5)
    assert all(torch.equal(u, v) for u, v in zip(first[0], second[0]))
    assert all(torch.equal(first[1][k], second[1][k]) for k in ("src", "dst"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_robust_variant(dtype):
    """The outlier set, seeds 0 to 7 as one batch, 10 reweighted solves at robust_scale 0.05: within 1e-9 max(1, S) of the restatement
    (values, final weights and the gradient at the final weights), and the true transform comes back where the plain solve misses it."""
    sets = [cases.outliers(seed) for seed in range(8)]
    c = dict(src=torch.cat([s["src"] for s in sets]), dst=torch.cat([s["dst"] for s in sets]), weights=None, mask=None)
    gpu, cpu = cast(c, dtype)
    kw = dict(robust_iters=10, robust_scale=0.05)
    want, want_w, want_g = ref.value_and_grads(cpu["src"], cpu["dst"], probes(8, 5, dtype), **kw)
    x, grads = run(gpu, dtype, probes(8, 5, dtype), ("src", "dst"), **kw)
    assert x.status.cpu().tolist() == want.status.tolist() == [ref.OK] * 8
    for name, n in (("R", 9), ("t", 3), ("s", 1), ("rms", 1)):
        close(getattr(x, name).reshape(8, n), getattr(want, name).reshape(8, n), dtype, f"robust {name}", factor=1e-9)
    for k in grads:
        close(grads[k].reshape(8, -1), want_g[k].reshape(8, -1), dtype, f"robust gradient on {k}", grad=True)
    _, w = _align().similarity_transform(gpu["src"], gpu["dst"], return_weights=True, **kw)
    close(w, want_w, torch.float64, "robust final weights", factor=1e-9)
    plain = _align().similarity_transform(gpu["src"], gpu["dst"])
    cpu_x = lambda y, b: ref.Transform(*(v[b:b + 1].cpu().double() for v in y))  # noqa: E731
    robust_err = max(cases.transform_error(cpu_x(x, b), sets[b]) for b in range(8))
    plain_err = min(cases.transform_error(cpu_x(plain, b), sets[b]) for b in range(8))
    print(f"outlier set on the GPU: robust max {robust_err:.3g}, plain min {plain_err:.3g}")
    assert robust_err <= 0.05 and plain_err >= 0.5


def errors_case():
    """(5,9,3): noisy copies under a transform; a sentinel target, a NaN prediction, an infinite target, masked joints, a sample with
    nothing valid and one with two valid joints."""
    c = cases.regular(5, 9, seed=21, weights=None, masked=False)
    pred, target = c["src"], c["dst"]
    mask = torch.ones(5, 9, dtype=torch.uint8)
    target[0, 1] = 0.0
    target[0, 2] = torch.tensor([3e-7, -3e-7, 0.0], dtype=torch.float64)  # within the sentinel's radius
    pred[1, 3, 2] = float("nan")
    target[1, 4, 0] = float("inf")
    mask[2, [0, 5]] = 0
    mask[3] = 0
    mask[4, 2:] = 0
    return pred, target, mask


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("sentinel", [True, False])
@pytest.mark.parametrize("mode", ["none", "rigid", "similarity"])
def test_joint_errors(mode, sentinel, dtype):
    a = _align()
    pred, target, mask = errors_case()
    p, t = pred.to(dtype), target.to(dtype)
    want_d, want_v, want_s = ref.joint_errors(p.double(), t.double(), mask, mode, sentinel)
    dist, valid, status = a.joint_errors(p.to(DEV), t.to(DEV), mask.to(DEV), mode, sentinel)
    assert valid.dtype == torch.bool and torch.equal(valid.cpu(), want_v)
    assert status.dtype == torch.int32 and status.cpu().tolist() == want_s.tolist()
    assert want_s.tolist()[3] == ref.EMPTY and (mode == "none" or want_s.tolist()[4] == ref.DEGENERATE)
    assert int(want_v[0].sum()) == (7 if sentinel else 9) and int(want_v[1].sum()) == 7 and int(want_v[2].sum()) == 7
    close(dist, want_d, dtype, f"joint_errors {mode} sentinel={sentinel}")
    assert not bool(dist[~valid].any())
    scaled, _, _ = a.joint_errors(p.to(DEV), t.to(DEV), mask.to(DEV), mode, sentinel, scale=1000.0)  # (the reference's 1 / world_scale)
    close(scaled, 1000.0 * want_d, dtype, f"joint_errors {mode} scale=1000")
    got = a.mpjpe(p.to(DEV), t.to(DEV), mask.to(DEV), sentinel) if mode == "none" else \
        a.pa_mpjpe(p.to(DEV), t.to(DEV), mask.to(DEV), mode == "similarity", sentinel)
    assert got.dim() == 0 and got.device.type == "cuda"
    close(got.reshape(1, 1), ref.pooled(want_d, want_v).reshape(1, 1), dtype, f"pooled {mode}")
    # without a mask, unbatched, and a batch with nothing valid
    d1, v1, s1 = a.joint_errors(p[2].to(DEV), t[2].to(DEV), None, mode, sentinel)
    w1 = ref.joint_errors(p[2:3].double(), t[2:3].double(), None, mode, sentinel)
    assert tuple(d1.shape) == (9,) and s1.dim() == 0 and torch.equal(v1.cpu(), w1[1][0])
    close(d1.reshape(1, 9), w1[0], dtype, f"joint_errors {mode} unbatched")
    assert float(a.pa_mpjpe(p[3:4].to(DEV), t[3:4].to(DEV), mask[3:4].to(DEV))) == 0.0
    assert float(a.mpjpe(p[3:4].to(DEV), t[3:4].to(DEV), mask[3:4].to(DEV))) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_pa_mpjpe_is_at_most_mpjpe_on_the_regular_set(dtype):
    a = _align()
    c = cases.regular(65, 63, seed=9, weights=None)
    gpu, cpu = cast(c, dtype)
    plain = a.mpjpe(gpu["src"], gpu["dst"], gpu["mask"])
    rigid = a.pa_mpjpe(gpu["src"], gpu["dst"], gpu["mask"], with_scale=False)
    full = a.pa_mpjpe(gpu["src"], gpu["dst"], gpu["mask"])
    print(f"mpjpe {float(plain):.6g}, rigid pa-mpjpe {float(rigid):.6g}, pa-mpjpe {float(full):.6g}")
    assert float(full) <= float(plain) and float(rigid) <= float(plain)
    close(full.reshape(1, 1), ref.pa_mpjpe(cpu["src"], cpu["dst"], cpu["mask"]).reshape(1, 1), dtype, "pa_mpjpe")
    close(plain.reshape(1, 1), ref.mpjpe(cpu["src"], cpu["dst"], cpu["mask"]).reshape(1, 1), dtype, "mpjpe")
    if dtype == torch.float64:  # the fused errors are the alignment applied: the two public paths agree (torch's own float32 would not do)
        x = a.similarity_transform(gpu["src"], gpu["dst"], mask=gpu["mask"])
        moved = a.apply_transform(gpu["src"], x.R, x.t, x.s)
        keep = gpu["mask"] != 0
        two_step = ((moved - gpu["dst"]).norm(dim=-1) * keep).sum() / keep.sum()
        close(full.reshape(1, 1), two_step.reshape(1, 1), dtype, "pa_mpjpe against apply_transform", factor=1e-9)


def test_refusals_on_the_device():
    a = _align()
    src, dst = torch.zeros(2, 5, 3, device=DEV), torch.ones(2, 5, 3, device=DEV)
    for kw in (dict(weights=torch.tensor([1.0, -1.0, 1, 1, 1], device=DEV)), dict(weights=torch.full((2, 5), float("nan"), device=DEV))):
        with pytest.raises(ValueError):
            a.similarity_transform(src, dst, **kw)
    from smilify_amd import _lib

    with pytest.raises(_lib.SmilError):
        a.similarity_transform(src, dst.cpu())
    with pytest.raises(_lib.SmilError):
        a.similarity_transform(src, dst, mask=torch.ones(2, 5))
    # unchecked, a weight that is not a positive finite number counts as 0
    w = torch.tensor([1.0, -1.0, float("nan"), 1.0, 1.0], device=DEV)
    x = a.similarity_transform(src, dst, weights=w, validate_weights=False)
    y = a.similarity_transform(src, dst, weights=torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0], device=DEV))
    assert all(torch.equal(u, v) for u, v in zip(x, y)) and x.status.cpu().tolist() == [ref.DEGENERATE] * 2


def test_global_pose_from_alignment_on_the_stick_model(tables):
    """A random joint pose, once under a global rotation of up to 3 rad and a translation, once under neither: the rigid alignment of
    the second joint set to the first, turned into a global-rotation row and trans, reproduces joints and vertices of the first within
    32 x 2^-24 max(1, largest |coordinate|) (the float32 rule of tests/test_gpu_keypoint_losses.py: LBS is float32)."""
    from smilify_amd.smal_torch import SMAL

    a = _align()
    t = tables("stick")
    smal = SMAL(DEV, tables=t)
    g = torch.Generator().manual_seed(4)
    B = 3
    beta = (0.5 * torch.randn(B, t.nB, generator=g)).to(DEV)
    theta = 0.3 * torch.randn(B, t.J, 3, generator=g)
    theta[:, 0] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1) * torch.tensor([0.4, 1.9, 3.0])[:, None]
    trans = torch.randn(B, 3, generator=g).to(DEV)
    theta = theta.to(DEV)
    rest = theta.clone()
    rest[:, 0] = 0.0
    verts1, joints1, _, _ = smal(beta, theta)
    verts1, joints1 = verts1 + trans[:, None], joints1 + trans[:, None]  # trans after the joints, as the fitter adds it
    _, joints0, _, _ = smal(beta, rest)
    x = a.rigid_transform(joints0, joints1)
    assert x.status.cpu().tolist() == [ref.OK] * B
    rot, tr = a.global_pose_from_alignment(smal, x.R, x.t, beta)
    assert tuple(rot.shape) == (B, 3) and tuple(tr.shape) == (B, 3) and rot.dtype == torch.float32
    posed = rest.clone()
    posed[:, 0] = rot
    verts2, joints2, _, _ = smal(beta, posed)
    verts2, joints2 = verts2 + tr[:, None], joints2 + tr[:, None]
    bound = 32 * 2.0 ** -24 * max(1.0, float(verts1.abs().max()), float(joints1.abs().max()))
    ev, ej = float((verts2 - verts1).abs().max()), float((joints2 - joints1).abs().max())
    print(f"global pose from alignment: vertices {ev:.3g}, joints {ej:.3g} (bound {bound:.3g}); rms {x.rms.cpu().tolist()}")
    assert ev <= bound and ej <= bound
    # the same through the root joint of the last call, and composed with a pose that already has a rotation and a translation
    rot_b, tr_b = a.global_pose_from_alignment(smal, x.R, x.t, root=smal.J_transformed[:, 0])
    assert float((rot_b - rot).abs().max()) <= 1e-6 and float((tr_b - tr).abs().max()) <= 1e-6
    back = a.rigid_transform(joints1, joints0)  # carries the posed joints home: the composed pose is the rest pose
    rot_c, tr_c = a.global_pose_from_alignment(smal, back.R, back.t, beta, global_rotation=theta[:, 0], trans=trans)
    assert float(rot_c.abs().max()) <= 2e-5 and float(tr_c.abs().max()) <= 2e-5
