"""The mesh-free joints kernels (smilify_amd/csrc/joints.hip: smil_joints_forward / smil_joints_backward) and ``SMAL.joints`` against
the float64 oracle (``lbs_ref64.reference``: dense LBS over every vertex, objective ``sum(joints * probe)``).

Bounds: ``row_err <= lbs_ref64.TOL[q]``, the project's own bounds for joints, new_J, d_beta, d_theta, d_trans, d_logscale, d_btrans;
against ``SMAL.__call__``'s joints ``2 TOL["joints"]`` (both lie within TOL of the same truth).  The kernels compute in float64 and
round once, so what they show is far inside (printed per case).

Shapes: J = 3 (smallest), 31 (mouse, static), 55 (STICK), 64 | 65 (one | two joints per lane), a random model above 128 joints (147:
three per lane), 250 (four per lane, more than 64 KB of LDS for one wave's backward), a
random model with a joint that regresses from more than 4 bones, static models (no pairs); B = 1, a block's frames +- 1 (a block holds
up to 4 frames, 3 in the backward of STICK), and 4 x 1024 + 3 frames, where the 1024 blocks loop over frames and a ragged last round
leaves waves idle.
"""
import pytest
import torch

import joints_cases
import lbs_ref64
from lbs_ref64 import TOL, row_err, rows_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("d_beta", "d_theta", "d_trans", "d_logscale", "d_btrans")

CASES = [
    # J and B
    ("j3-B1", "j3", dict(B=1, seed=1)),
    ("mouse-B3", "mouse", dict(B=3, seed=2)),
    ("mouse-B5-call", "mouse", dict(B=5, seed=3, trans_after_joints=False)),
    ("stick-B2", "stick", dict(B=2, seed=4)),
    ("stick-B4", "stick", dict(B=4, seed=5)),
    ("stick-B5", "stick", dict(B=5, seed=6)),
    ("j64-B3", "j64", dict(B=3, seed=7)),
    ("j65-B5", "j65", dict(B=5, seed=8)),
    ("j65-static-B4", "j65_static", dict(B=4, seed=9)),
    ("wide-B2", "random_wide", dict(B=2, seed=10)),
    ("j250-B2", "j250", dict(B=2, seed=15)),  # four joints per lane; a wave's backward tables (78 KB) pass 64 KB of LDS
    ("many-bones-B3", "random", dict(B=3, seed=11)),
    ("static-B5", "synthetic_static", dict(B=5, seed=12)),
    ("loop-B4099", "synthetic", dict(B=4099, seed=13)),
    ("loop-B4099-perframe", "synthetic_static", dict(B=4099, seed=14, shared_beta=False, logscale_shared=False, btrans_shared=False)),
    # options
    ("perframe-beta", "stick", dict(B=5, seed=20, shared_beta=False)),
    ("nB_used0", "synthetic", dict(B=5, seed=21, nB_used=0)),
    ("nB_used2", "synthetic", dict(B=5, seed=22, nB_used=2)),
    ("nB_used2-perframe", "synthetic", dict(B=5, seed=23, nB_used=2, shared_beta=False)),
    ("tables-absent", "stick", dict(B=5, seed=24, logscale=False, btrans=False)),
    ("tables-perframe", "stick", dict(B=5, seed=25, logscale_shared=False, btrans_shared=False, ls_scale=0.3)),
    ("no-limb-scaling", "stick", dict(B=5, seed=26, allow_limb_scaling=False, ls_scale=0.5)),
    ("propagate", "stick", dict(B=5, seed=27, propagate_scaling=True, ls_scale=0.3)),
    ("propagate-perframe", "synthetic", dict(B=5, seed=28, propagate_scaling=True, logscale_shared=False, ls_scale=0.3)),
    ("call-convention", "stick", dict(B=5, seed=29, trans_after_joints=False)),
    ("mask", "stick", dict(B=5, seed=30, mask=True)),
    ("mask-static", "synthetic_static", dict(B=5, seed=31, mask=True)),
    ("edge-theta", "stick", dict(B=8, seed=32, theta="edge", logscale_shared=False)),
    ("edge-theta-static", "mouse", dict(B=8, seed=33, theta="edge", ls_scale=0.3)),
]


def _engine():
    from smilify_amd import engine
    from smilify_amd.joints import JointTables

    return engine, JointTables


_TABLES = {}


def _device_tables(key, tables):
    if key not in _TABLES:
        eng, JointTables = _engine()
        t = joints_cases.get_model(key, tables)
        _TABLES[key] = (t, eng.DeviceJointTables(JointTables.from_tables(t), DEV))
    return _TABLES[key]


def _args(case, with_trans=True):
    inp, fl = case["inp"], case["fl"]
    cu = lambda x: None if x is None else x.to(DEV).contiguous()  # noqa: E731
    pos = (cu(inp["beta"]), cu(inp["theta"]), cu(inp["trans"]) if with_trans else None, cu(inp.get("ls")), cu(inp.get("bt")),
           cu(inp.get("theta_mask")))
    flags = dict(trans_after_joints=fl["trans_after_joints"], propagate_scaling=fl["propagate_scaling"], allow_limb_scaling=fl["allow_limb_scaling"])
    return pos, flags


def _check(name, got, want, case, keys):
    worst = {}
    for k in keys:
        e = row_err(got[k], want[k], rows_of(k, case))
        worst[k] = e
        assert e <= TOL[k], f"{name}: {k} row error {e:.3e} above {TOL[k]:.1e}"
    print(f"[joints] {name}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("name,key,kw", CASES, ids=[c[0] for c in CASES])
def test_kernels_against_oracle(tables, name, key, kw):
    eng, _ = _engine()
    t, jt = _device_tables(key, tables)
    case = joints_cases.joints_case(t, **kw)
    fwd, grads = lbs_ref64.reference(t, case)
    pos, flags = _args(case)
    joints, new_J = eng.joints_forward(jt, *pos, **flags)
    _check(name, dict(joints=joints, new_J=new_J), fwd, case, ("joints", "new_J"))
    need = [k for k in GRADS if k in grads]
    got = eng.joints_backward(jt, case["up"]["d_joints"].to(DEV), *pos, need=need, **flags)
    assert set(got) == set(need)
    _check(name, got, grads, case, need)


def test_trans_none(tables):
    """No translation: the joints of a zero translation, and the other gradients unchanged."""
    eng, _ = _engine()
    t, jt = _device_tables("stick", tables)
    case = joints_cases.joints_case(t, B=5, seed=40)
    case["inp"]["trans"] = torch.zeros(5, 3)
    fwd, grads = lbs_ref64.reference(t, case)
    pos, flags = _args(case, with_trans=False)
    joints, new_J = eng.joints_forward(jt, *pos, **flags)
    _check("trans-none", dict(joints=joints, new_J=new_J), fwd, case, ("joints", "new_J"))
    need = [k for k in GRADS if k != "d_trans"]
    _check("trans-none", eng.joints_backward(jt, case["up"]["d_joints"].to(DEV), *pos, need=need, **flags), grads, case, need)
    got = eng.joints_backward(jt, case["up"]["d_joints"].to(DEV), *pos, need=["d_trans"], **flags)
    assert not got["d_trans"].any()  # (a translation that is not there has no effect)


@pytest.mark.parametrize("key,B", [("stick", 5), ("synthetic", 4099)])
def test_shared_gradients_reproducible_and_outputs_skippable(tables, key, B):
    """Two backward calls give the same bits for every gradient (the sums over frames of the shared tables included), and a call that
    asks for one gradient returns the bits the full call returned for it."""
    eng, _ = _engine()
    t, jt = _device_tables(key, tables)
    case = joints_cases.joints_case(t, B=B, seed=50)
    pos, flags = _args(case)
    dj = case["up"]["d_joints"].to(DEV)
    a = eng.joints_backward(jt, dj, *pos, need=GRADS, **flags)
    b = eng.joints_backward(jt, dj, *pos, need=GRADS, **flags)
    for k in GRADS:
        assert torch.equal(a[k], b[k]), f"{k} differs between two calls"
    assert a["d_beta"].dim() == 1 and a["d_logscale"].shape == (t.J, 3) and a["d_btrans"].shape == (t.J, 3)
    for k in GRADS:
        one = eng.joints_backward(jt, dj, *pos, need=[k], **flags)
        assert list(one) == [k] and torch.equal(one[k], a[k]), f"{k} alone differs from {k} of the full call"


def test_bad_arguments(tables):
    eng, _ = _engine()
    from smilify_amd import _lib

    t, jt = _device_tables("synthetic", tables)
    case = joints_cases.joints_case(t, B=3, seed=60)
    pos, flags = _args(case)
    with pytest.raises(ValueError):
        eng.joints_forward(jt, pos[0], pos[1][:, :-1].contiguous(), *pos[2:], **flags)
    with pytest.raises(ValueError):
        eng.joints_forward(jt, torch.zeros(t.nB + 1, device=DEV), *pos[1:], **flags)
    lib = _lib.load()
    import ctypes

    i = _lib.JointsInputs()  # B = 0, no theta
    assert lib.smil_joints_forward(ctypes.byref(jt.struct), ctypes.byref(i), None, None, None) == -1
    assert b"smil_joints_forward" in lib.smil_last_error()


@pytest.mark.parametrize("key", ["stick", "mouse", "synthetic"])
def test_smal_joints(tables, key):
    """``SMAL.joints`` against the oracle (forward and autograd) and against ``SMAL.__call__``, shared and per-frame inputs."""
    from smilify_amd.smal_torch import SMAL

    t = joints_cases.get_model(key, tables)
    smal = SMAL(DEV, tables=t)
    for shared in (True, False):
        B = 5
        case = joints_cases.joints_case(t, B=B, seed=70 + shared, trans_after_joints=False, shared_beta=shared, logscale_shared=shared,
                                        btrans_shared=shared)
        fwd, grads = lbs_ref64.reference(t, case)
        inp = case["inp"]
        leaf = lambda x: x.to(DEV).clone().requires_grad_()  # noqa: E731
        beta = leaf(inp["beta"][None] if shared else inp["beta"])
        theta, trans = leaf(inp["theta"]), leaf(inp["trans"])
        ls, bt = leaf(inp["ls"][None] if shared else inp["ls"]), leaf(inp["bt"][None] if shared else inp["bt"])
        joints = smal.joints(beta, theta, trans, betas_logscale=ls, betas_trans=bt)
        assert joints.shape == (B, t.J, 3) and joints.requires_grad
        got = dict(joints=joints, new_J=smal.J_transformed)
        (joints * case["up"]["d_joints"].to(DEV)).sum().backward()
        got.update(d_beta=beta.grad, d_theta=theta.grad, d_trans=trans.grad, d_logscale=ls.grad, d_btrans=bt.grad)
        assert beta.grad.shape == beta.shape and ls.grad.shape == ls.shape and bt.grad.shape == bt.shape
        _check(f"SMAL.joints[{key}-shared{int(shared)}]", got, dict(fwd, **grads), case, ("joints", "new_J") + GRADS)
        with torch.no_grad():
            _, ref_joints, _, _ = smal(beta, theta, trans, betas_logscale=ls, betas_trans=bt)
        e = row_err(joints, ref_joints, B)
        print(f"[joints] SMAL.joints[{key}] against SMAL.__call__: {e:.1e}")
        assert e <= 2 * TOL["joints"]
        assert row_err(smal.J_transformed, fwd["new_J"], B) <= TOL["new_J"]
    with pytest.raises(ValueError, match="__call__"):
        smal.joints(beta, torch.zeros(5, t.J, 3, 3, device=DEV))
