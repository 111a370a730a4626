"""The host side of the mesh-free joints path without a GPU: ``smilify_amd.joints.JointTables`` against the float64 oracle
(``lbs_ref64.reference``: dense LBS over every vertex), and the float64 restatement of the 3-D keypoint term (tests/joints_ref.py)
against central finite differences.

Bound of the moments: a joint is a sum of at most nnz x 4 (STICK: about 6 200) float64 products of one sign pattern, so the row error is
at most that many times 2^-53 = 7e-13 < 1e-12.  Measured: 4.2e-16 (STICK) .. 1.3e-15.
"""
import itertools

import numpy as np
import pytest
import torch

import joints_cases
import joints_ref
import lbs_ref64
from smilify_amd.joints import JointTables

MOMENT_TOL = 1e-12
MODELS = ("stick", "synthetic", "synthetic_static", "random", "random_wide")


@pytest.mark.parametrize("after,prop", list(itertools.product((True, False), (False, True))))
@pytest.mark.parametrize("key", MODELS)
def test_moments_against_oracle(tables, key, after, prop):
    t = joints_cases.get_model(key, tables)
    jt = JointTables.from_tables(t)
    assert (jt.P == 0) == bool(t.static_joints)
    case = joints_cases.joints_case(t, B=3, seed=5 + 2 * after + prop, trans_after_joints=after, propagate_scaling=prop, ls_scale=0.2)
    fwd, _ = lbs_ref64.reference(t, case)
    inp = case["inp"]
    beta = inp["beta"].double().numpy()
    got_rest = jt.rest_joints(beta)
    got = jt.joints_from_transforms(fwd["A"].numpy(), beta, inp["trans"].double().numpy(), trans_after_joints=after)
    m = lbs_ref64.dense_model(t)
    want_rest = m["J_static"] if t.static_joints else torch.einsum("vj,vc->jc", m["J_regressor"],
                                                                     m["v_template"] + (inp["beta"].double() @ m["shapedirs"]).view(-1, 3))
    e_rest = lbs_ref64.row_err(got_rest[0], want_rest, 1)
    e = lbs_ref64.row_err(got, fwd["joints"], 3)
    print(f"[joints-cpu] {key} after={after} prop={prop}: P={jt.P} max pairs/joint={int(np.diff(jt.pair_ptr).max())} "
          f"row error joints {e:.2e} rest {e_rest:.2e}")
    assert e <= MOMENT_TOL and e_rest <= MOMENT_TOL


def test_stick_pair_count(tables):
    jt = JointTables.from_tables(tables("stick"))
    assert jt.P == 114 and int(np.diff(jt.pair_ptr).max()) <= 4
    assert np.abs(jt.rowsum - 1).max() < 1e-6 and (jt.rowsum != 1).any()  # (not exactly 1: trans before the regression needs it)


def test_raises_for_unsupported(tables):
    with pytest.raises(NotImplementedError, match="posedirs"):
        JointTables.from_tables(lbs_ref64.get_tables("posedirs"))
    t = tables("synthetic")
    with pytest.raises(NotImplementedError, match="del_v"):
        JointTables.from_tables(t, del_v=np.zeros((t.V, 3), np.float32))
    with pytest.raises(NotImplementedError, match="v_template"):
        JointTables.from_tables(t, v_template=t.v_template)


@pytest.mark.parametrize("key", MODELS)
def test_pair_orders_hold_the_same_set(tables, key):
    jt = JointTables.from_tables(joints_cases.get_model(key, tables))
    J = jt.J
    by_joint = [(j, int(k)) for j in range(J) for k in jt.pair_bone[jt.pair_ptr[j]:jt.pair_ptr[j + 1]]]
    by_bone = [(int(j), k) for k in range(J) for j in jt.bpair_joint[jt.bpair_ptr[k]:jt.bpair_ptr[k + 1]]]
    assert len(by_joint) == jt.P == len(set(by_joint)) and sorted(by_joint) == sorted(by_bone)
    for k in range(J):  # the index of a by-bone entry names the same pair in the by-joint order
        for e in range(jt.bpair_ptr[k], jt.bpair_ptr[k + 1]):
            assert by_joint[jt.bpair_index[e]] == (int(jt.bpair_joint[e]), k)
    kids = [[int(c) for c in jt.child[jt.child_ptr[j]:jt.child_ptr[j + 1]]] for j in range(J)]
    assert all(jt.parents[c] == j for j in range(J) for c in kids[j]) and sum(map(len, kids)) == J - 1
    assert all(k == sorted(k) for k in kids)


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_term_against_finite_differences(sigma):
    """rho, the sentinel, NaN rows, visibility, weights and window means with N % window != 0."""
    g = torch.Generator().manual_seed(3)
    N, J, Jc, window = 7, 9, 5, 3
    canon = [6, 2, 8, 0, 3]
    joints = torch.randn(N, J, 3, generator=g, dtype=torch.float64)
    target = (joints[:, canon] + 0.1 * torch.randn(N, Jc, 3, generator=g, dtype=torch.float64)).float()
    target[0, 1] = 0.0                       # sentinel
    target[2, 3, 1] = float("nan")           # failed triangulation
    target[4] = 0.0                          # a frame with nothing visible
    target[5, 0] += 3.0                      # far beyond sigma
    vis = torch.ones(N, Jc, dtype=torch.uint8)
    vis[1, 2] = 0
    wj = torch.tensor([1.0, 0.5, 2.0, 0.0, 1.5], dtype=torch.float64)
    f = lambda x: joints_ref.kp3d_term(x, target, vis, wj, canon, 7.0, sigma, window)  # noqa: E731
    x = joints.clone().requires_grad_()
    val = f(x)
    val.backward()
    seen = joints_ref.visible(target, vis)
    assert not seen[0, 1] and not seen[2, 3] and not seen[4].any() and not seen[1, 2] and int(seen.sum()) == N * Jc - 8
    # the term by hand for one entry: frames 0-2 form a window of 3, frame 6 one of 1
    s = ((joints[6, canon[0]] - target[6, 0].double()) ** 2).sum()
    rho = s if sigma == 0 else 2 * sigma ** 2 * (torch.sqrt(1 + s / sigma ** 2) - 1)
    only = torch.zeros(N, Jc, dtype=torch.uint8)
    only[6, 0] = 1
    assert torch.allclose(joints_ref.kp3d_term(joints, target, only, wj, canon, 7.0, sigma, window), 7.0 * wj[0] * rho / (3 * Jc * 1), rtol=1e-14)
    assert not x.grad[4].any() and not x.grad[:, [1, 4, 5, 7]].any()  # nothing visible / joints outside canon: exactly zero
    h = 1e-6
    flat = joints.reshape(-1)
    worst = 0.0
    for i in range(flat.numel()):
        d = torch.zeros_like(flat)
        d[i] = h
        fd = (f((flat + d).view_as(joints)) - f((flat - d).view_as(joints))) / (2 * h)
        worst = max(worst, abs(fd.item() - x.grad.reshape(-1)[i].item()))
    # central differences: error ~ h^2 f''' / 6 + eps |f| / h; with |f| ~ 10, h = 1e-6: 2e-9
    assert worst <= 1e-7 * max(1.0, x.grad.abs().max().item()), worst
