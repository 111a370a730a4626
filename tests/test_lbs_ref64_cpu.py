"""CPU checks of the float64 LBS / projection references of tests/lbs_ref64.py (no GPU): they reproduce the vectors of the real
reference, their autograd agrees with central finite differences at every pose edge, the fp32 oracle stays within TOL / 16 of
them on every case family of tests/test_gpu_lbs_float64.py (the measurement the bounds are derived from), and the packed
fixed-point encoder round-trips through a restatement of the kernels' decode."""
import math

import numpy as np
import pytest
import torch

import lbs_ref64 as r64
from conftest import vertex_probe
from oracle import lbs_ref

F64 = torch.float64


def _np(x):
    return x.detach().numpy()


@pytest.mark.parametrize("key", ["stick", "mouse"])
def test_float64_reference_reproduces_the_real_reference_goldens(key, golden, tables):
    """lbs_<key>.npz and lbs_extra_<key>.npz at the bounds tests/test_oracle_lbs.py and tests/test_gpu_smal_api.py use."""
    g = golden(f"lbs_{key}")
    m = r64.dense_model(tables(key))
    leaf = {n: torch.from_numpy(g[f"smal_{n}"]).to(F64).requires_grad_() for n in ["beta", "theta", "trans", "ls", "bt"]}
    out = lbs_ref.smal_forward(m, leaf["beta"], leaf["theta"], trans=leaf["trans"], betas_logscale=leaf["ls"], betas_trans=leaf["bt"])
    assert out["verts"].dtype == F64
    np.testing.assert_allclose(_np(out["verts"]), g["smal_verts"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(_np(out["joints"]), g["smal_joints"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(_np(out["Rs"]), g["smal_Rs"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_np(out["v_shaped"]), g["smal_v_shaped"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_np(out["new_J"]), g["smal_J_transformed"], rtol=1e-4, atol=2e-6)
    ((out["verts"] * vertex_probe(out["verts"].shape, 0)).sum() + (out["joints"] * vertex_probe(out["joints"].shape, 1)).sum()).backward()
    for n, t in leaf.items():
        ref = g[f"smal_grad_{n}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(t.grad.numpy() / scale, ref / scale, rtol=0, atol=2e-4, err_msg=n)
    # del_v, rotation-matrix pose, one-row trans / log-scales
    g = golden(f"lbs_extra_{key}")
    leaf = {n: torch.from_numpy(g[n]).to(F64).requires_grad_() for n in ("beta", "Rs", "trans", "del_v", "ls", "bt")}
    B = leaf["beta"].shape[0]
    out = lbs_ref.smal_forward(m, leaf["beta"], leaf["Rs"], trans=leaf["trans"].expand(B, -1), del_v=leaf["del_v"],
                               betas_logscale=leaf["ls"].expand(B, -1, -1), betas_trans=leaf["bt"])
    np.testing.assert_allclose(_np(out["verts"]), g["verts"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(_np(out["joints"]), g["joints"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(_np(out["v_shaped"]), g["v_shaped"], rtol=2e-5, atol=2e-6)
    ((out["verts"] * vertex_probe(out["verts"].shape, 2)).sum() + (out["joints"] * vertex_probe(out["joints"].shape, 3)).sum()).backward()
    for n, t in leaf.items():
        ref = g[f"grad_{n}"]
        scale = np.abs(ref).max() + 1e-12
        np.testing.assert_allclose(t.grad.numpy() / scale, ref / scale, rtol=0, atol=3e-4, err_msg=n)


def test_float64_reference_reproduces_the_pose_blend_golden(golden):
    g = golden("lbs_posedirs")
    m = r64.dense_model(r64.get_tables("posedirs"))
    leaves = {n: torch.from_numpy(g[n]).to(F64).requires_grad_() for n in ("beta", "theta", "trans")}
    out = lbs_ref.smal_forward(m, leaves["beta"], leaves["theta"], trans=leaves["trans"])
    np.testing.assert_allclose(_np(out["verts"]), g["verts"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(_np(out["joints"]), g["joints"], rtol=1e-4, atol=2e-6)
    ((out["verts"] * vertex_probe(out["verts"].shape, 0)).sum() + (out["joints"] * vertex_probe(out["joints"].shape, 1)).sum()).backward()
    for n in leaves:
        ref = g[f"grad_{n}"]
        sc = np.abs(ref).max()
        np.testing.assert_allclose(leaves[n].grad.numpy() / sc, ref / sc, atol=2e-4, err_msg=n)


@pytest.mark.parametrize("ls_scale", [0.3, 1.0])
def test_float64_autograd_agrees_with_central_differences_at_every_pose_edge(ls_scale, tables):
    """Every row of ``edge_theta`` (theta = 0, 1e-6, 1e-3, |theta| = pi - 1e-3, pi, pi + 0.5, 2 pi + 0.1, single axis): the
    directional derivative of the objective along a random direction in (theta, log-scales, trans, beta) of that frame, by
    central differences in float64 (steps 1e-6 and 1e-7 - the tiny-theta rows have curvature of order 1 / |theta + 1e-8|),
    against the autograd gradients.  Bound 1e-5 of the derivative: truncation h^2 f''' / 6 and rounding 1e-16 |f| / h of a
    float64 central difference are both below it for the better of the two steps."""
    t = tables("synthetic_static")
    case = r64.build_case(t, dict(B=8, seed=5, theta="edge", ls_scale=ls_scale, logscale_shared=False, shared_beta=False))
    _, grads = r64.reference(t, case)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    g = torch.Generator().manual_seed(9)
    names = dict(theta="d_theta", ls="d_logscale", trans="d_trans", beta="d_beta")
    dirs = {k: torch.randn(case["inp"][k].shape, generator=g, dtype=F64) for k in names}

    def objective(step, frame):
        c = dict(case, inp={k: v.to(F64) for k, v in case["inp"].items()})
        for k in names:
            x = c["inp"][k].clone()
            x[frame] += step * dirs[k][frame]
            c["inp"][k] = x
        m = r64.dense_model(t)
        o = lbs_ref.smal_forward(m, c["inp"]["beta"], c["inp"]["theta"], betas_logscale=c["inp"]["ls"],
                                 betas_trans=c["inp"]["bt"][None].expand(8, -1, -1))
        v, j = o["verts"] + c["inp"]["trans"][:, None], o["joints"] + c["inp"]["trans"][:, None]
        return float((v * case["up"]["d_verts"].to(F64)).sum() + (j * case["up"]["d_joints"].to(F64)).sum())

    for frame in range(8):
        want = sum(float((grads[n][frame] * dirs[k][frame]).sum()) for k, n in names.items())
        errs = []
        for h in (1e-6, 1e-7):
            fd = (objective(h, frame) - objective(-h, frame)) / (2 * h)
            errs.append(abs(fd - want) / abs(want))
        print(f"frame {frame}: d = {want:.6e}, finite-difference error {errs}")
        assert min(errs) < 1e-5, (frame, want, errs)


def _oracle32_errors(t, case):
    f64, g64 = r64.reference(t, case, torch.float64)
    f32, g32 = r64.reference(t, case, torch.float32)
    return {k: r64.row_err(v, {**f64, **g64}[k], r64.rows_of(k, case)) for k, v in {**f32, **g32}.items()}


def _cpu_specs():
    """Every family; of the batch family the sizes a CPU walks in seconds (the error of the fp32 oracle grows with B only in
    the sums over frames, which the largest size shows)."""
    fam = r64.lbs_specs()
    keep = ("stick-B1-v1", "stick-B65-v2", "stick-B255-v1", "stick-B259-v1", "stick-B1027-v2", "stick-perframe-B259", "mouse-B3", "mouse-B257", "stick-perframe-B65")
    out = [("batch",) + s for s in fam["batch"] if s[0] in keep]
    return out + [("options",) + s for s in fam["options"]] + [("pose",) + s for s in fam["pose"]]


@pytest.mark.parametrize("family,cid,key,kw", _cpu_specs(), ids=lambda v: v if isinstance(v, str) else "")
def test_fp32_oracle_stays_within_a_sixteenth_of_the_bounds(family, cid, key, kw, tables):
    """The measurement ``lbs_ref64.MEASURED`` / ``TOL`` are derived from, kept alive: row_err(fp32 oracle, float64 oracle)
    for every quantity of every case family <= TOL / MARGIN."""
    t = r64.get_tables(key, tables)
    errs = _oracle32_errors(t, r64.build_case(t, kw))
    print(family, cid, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= r64.MEASURED[k], (k, v, r64.MEASURED[k])
        assert r64.TOL[k] <= r64.MARGIN[k] * r64.MEASURED[k] and r64.MARGIN[k] <= 64


@pytest.mark.parametrize("cid,kw", r64.projection_specs(), ids=lambda v: v if isinstance(v, str) else "")
def test_fp32_projection_stays_within_a_sixteenth_of_the_bounds(cid, kw):
    c = r64.make_projection_case(**kw)
    f64, g64, fov64 = r64.projection_reference(c, torch.float64)
    f32, g32, fov32 = r64.projection_reference(c, torch.float32)
    sfx = "_near" if c["near"] else ""
    errs = {}
    for a, b in zip(f32 + g32, f64 + g64):
        for k in a:
            errs[k + sfx] = max(errs.get(k + sfx, 0.0), r64.row_err(a[k], b[k], c["frames"]))
    errs["d_fov" + sfx] = r64.row_err(fov32, fov64, c["frames"] if fov64.numel() == c["frames"] * c["views"] else 1)
    print(cid, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= r64.MEASURED[k], (k, v, r64.MEASURED[k])


def test_bounds_respect_the_ceilings_of_the_older_tests():
    for k, v in r64.TOL.items():
        assert v <= (r64.GRAD_CEILING if k.startswith("d_") else r64.FWD_CEILING), k
        assert 16 <= r64.MARGIN[k] <= 64, k


def test_row_err_is_per_row_and_exact_on_zero_rows():
    want = torch.tensor([[1.0, 2.0], [1e-6, 0.0], [0.0, 0.0]])
    assert r64.row_err(want, want, 3) == 0.0
    got = want.clone()
    got[1, 0] = 2e-6  # wholly wrong, and invisible to a metric that divides by the global largest component
    assert r64.row_err(got, want, 3) == pytest.approx(1.0) and r64.row_err(got, want, 1) < 1e-6
    got = want.clone()
    got[2, 1] = 1e-30
    assert r64.row_err(got, want, 3) == math.inf
    got = want.clone()
    got[0, 0] = float("nan")
    assert r64.row_err(got, want, 3) == math.inf


def test_packed_encoder_round_trips_through_the_decode():
    g = torch.Generator().manual_seed(1)
    grad = (1e-3 * torch.randn(5, 300, 2, generator=g)).numpy().astype(np.float64)
    grad[0, 0] = (0.0, -2.0 ** -30)      # y = -1: every low bit set, the high half borrows one from x = 0
    grad[0, 1] = (-2.0 ** -30, 2.0 ** -30)
    grad[0, 2] = (3 * 2.0 ** -30, -(2 ** 31 - 1) * 2.0 ** -30)
    scale = np.array([2.0 ** -30, 0.0, 2.0 ** -30, 2.0 ** -34, 0.0], np.float32)
    grad[3] *= 2.0 ** -4
    words, decoded = r64.encode_packed(grad, scale)
    assert words.dtype == torch.float32 and tuple(words.shape) == (5, 300, 2)
    back = r64.decode_packed_np(words, scale)
    np.testing.assert_array_equal(back, decoded.numpy())
    assert (decoded.numpy()[..., 1] < 0).any() and (decoded.numpy()[..., 0] < 0).any()
    # quantisation: half a step at the most on packed rows, fp32 rounding on plain rows
    for n in range(5):
        step = scale[n] if scale[n] > 0 else 1e-10
        assert np.abs(decoded.numpy()[n] - grad[n]).max() <= 0.5 * step + 1e-12
    w = np.ascontiguousarray(words.numpy()).view(np.int32).reshape(5, 300, 2)
    assert w[0, 0, 0] == -1 and w[0, 0, 1] == -1      # (x = 0, y = -1) is the word -1
    assert w[0, 1, 0] == 1 and w[0, 1, 1] == -1       # (x = -1, y = 1)
    assert w[0, 2, 1] == 2 and w[0, 2, 0] == -(2 ** 31 - 1)
