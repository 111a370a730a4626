"""The point refinement kernels (csrc/refine_points.hip) on the GPU at their edges: one accumulation (cost, g, H) against the 40-digit
evaluation of tests/refine_points_ref.py with numpy's own error as the yardstick, error <= max(4 x numpy's, 2^-45) in units of the
largest entry; batches of 1, 4, 5 and 509 problems (one workgroup, the workgroup's edge, 128 workgroups) with a problem alone giving
the bits it gives inside the batch; and every status."""
import numpy as np
import pytest

import refine_points_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -45
OFFSET = np.array([0.03, -0.02, 0.05])  # off the minimum: there g is large, at the DLT start it is the small rest of a cancellation


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.parametrize("g", ["v2", "v3", "v12", "v32"])
@pytest.mark.parametrize("where", ["start", "offset"])
def test_one_accumulation_against_40_digits(fx, g, where):
    """C = 2, 3, 12, 32; in v12 and v32 masks without the lowest bit, without the highest, without both, and with five or fifteen
    views dropped in the middle; the dropped views' observations are NaN."""
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = R.group(fx, g)
    X = xyz0 + (OFFSET if where == "offset" else 0.0)
    out = rp.evaluate_points_cost(P, obs, mask, X, float(fx["f_scale"]))
    if g in ("v12", "v32"):
        C = len(P)
        assert [int(m) & 1 for m in mask[1:4, 0]] == [0, 1, 0] and [(int(m) >> (C - 1)) & 1 for m in mask[1:4, 0]] == [1, 0, 0]
        assert np.isnan(obs[1, 0, 0]).all() and np.isnan(obs[2, 0, C - 1]).all()
    for i in range(len(obs)):
        exact, own = R.high_precision((g, where, i), P, obs[i, 0], mask[i, 0], X[i, 0], float(fx["f_scale"]))
        e_gpu, e_np = R.errors((out[0][i, 0], out[1][i, 0], out[2][i, 0]), exact), R.errors(own, exact)
        print(f"accuracy {g} {where} problem {i} ({len(R.views_of(mask[i, 0], len(P)))} views): gpu cost {e_gpu[0]:.2e} g {e_gpu[1]:.2e} "
              f"H {e_gpu[2]:.2e} | numpy cost {e_np[0]:.2e} g {e_np[1]:.2e} H {e_np[2]:.2e}")
        for got, yard in zip(e_gpu, e_np):
            assert got <= max(4.0 * yard, FLOOR), (g, where, i, e_gpu, e_np)
        assert np.array_equal(out[2][i, 0], out[2][i, 0].T)


@pytest.fixture(scope="module")
def batch(fx):
    """509 problems of 12 cameras: the fixture's ring12 problems over and over, every start moved by its own seeded millimetres; the fit
    and one accumulation of the whole batch, once."""
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = R.group(fx, "ring12")
    idx = np.arange(509) % len(obs)
    xyz = xyz0[idx] + np.random.default_rng(7).normal(0.0, 2e-3, (509, 1, 3))
    inputs = (P, np.ascontiguousarray(obs[idx]), np.ascontiguousarray(mask[idx]), xyz)
    return inputs, rp.refine_points_arrays(*inputs), rp.evaluate_points_cost(*inputs)


def same_fit(a, b, sl):
    return np.array_equal(a[0], b[0][sl]) and all(np.array_equal(a[1][k], b[1][k][sl], equal_nan=True) for k in a[1])


@pytest.mark.parametrize("count", [1, 4, 5, 509])
def test_batch_sizes_and_two_runs(batch, count):
    """The first `count` problems as a batch of their own give the bits they give inside the 509 (count = 509: a second run)."""
    from smilify_amd import refine_points as rp

    (P, obs, mask, xyz), fit, ev = batch
    again = rp.refine_points_arrays(P, obs[:count], mask[:count], xyz[:count])
    assert same_fit(again, fit, slice(0, count))
    ev2 = rp.evaluate_points_cost(P, obs[:count], mask[:count], xyz[:count])
    assert all(np.array_equal(a, b[:count]) for a, b in zip(ev2, ev))
    assert (fit[1]["status"] <= R.STEP_LIMIT).all() and (fit[1]["cost_final"] <= fit[1]["cost_initial"]).all()
    assert (fit[1]["n_trials"] >= 2).all() and (fit[1]["n_accepted"] < fit[1]["n_trials"]).all()


@pytest.mark.parametrize("i", [3, 4, 300, 508])
def test_a_problem_alone_gives_the_bits_of_the_batch(batch, i):
    """Wave 3 and wave 0 of a workgroup, the middle of the grid and its last, partly filled workgroup."""
    from smilify_amd import refine_points as rp

    (P, obs, mask, xyz), fit, ev = batch
    alone = rp.refine_points_arrays(P, obs[i:i + 1], mask[i:i + 1], xyz[i:i + 1])
    assert same_fit(alone, fit, slice(i, i + 1))
    assert all(np.array_equal(a, b[i:i + 1]) for a, b in zip(rp.evaluate_points_cost(P, obs[i:i + 1], mask[i:i + 1], xyz[i:i + 1]), ev))


def test_every_status_and_the_neighbours_of_a_failed_problem(fx):
    """Eight problems, two workgroups: a one-view mask and an empty mask give status 2, a NaN start and a start on a camera's
    h2 = 0 plane status 3, all four with xyz unchanged to the bit; the four healthy problems between them are what they are alone."""
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = (a.copy() for a in R.group(fx, "v3"))
    P[1, 2] = [0.0, 0.0, 1.0, 0.0]  # camera 1: h2 = z exactly
    take = np.array([1, 2, 3, 4, 5, 1, 2, 3])
    obs, mask, xyz = obs[take], mask[take], xyz0[take]
    mask[1, 0], mask[3, 0] = 1 << 2, 0  # one view, no view
    xyz[4, 0, 1] = np.nan               # a failed triangulation
    xyz[6, 0, 2] = 0.0                  # on camera 1's plane: h / 0
    bad, good = [1, 3, 4, 6], [0, 2, 5, 7]
    out, st = rp.refine_points_arrays(P, obs, mask, xyz)
    assert st["status"].ravel().tolist() == [st["status"][0, 0], 2, st["status"][2, 0], 2, 3, st["status"][5, 0], 3, st["status"][7, 0]]
    assert (st["status"][good] <= R.STEP_LIMIT).all()
    assert np.array_equal(out[bad].view(np.int64), xyz[bad].view(np.int64))  # unchanged, the NaN's bits included
    assert (st["n_trials"][[1, 3], 0] == 0).all() and (st["n_trials"][[4, 6], 0] == 1).all() and (st["n_accepted"][bad] == 0).all()
    assert np.isnan(st["cost_initial"][[1, 3]]).all() and np.isnan(st["cost_final"][[1, 3]]).all()
    assert not np.isfinite(st["cost_initial"][[4, 6]]).any() and not np.isfinite(st["cost_final"][[4, 6]]).any()
    assert np.isnan(st["view_err"][1, 0, :2]).all() and np.isfinite(st["view_err"][1, 0, 2]) and np.isnan(st["view_err"][3, 0]).all()
    for i in good:
        alone = rp.refine_points_arrays(P, obs[i:i + 1], mask[i:i + 1], xyz[i:i + 1])
        assert same_fit(alone, (out, st), slice(i, i + 1)), i
        assert st["cost_final"][i, 0] <= st["cost_initial"][i, 0] and st["n_trials"][i, 0] >= 2
    ev = rp.evaluate_points_cost(P, obs, mask, xyz)
    assert ev[0][3, 0] == 0.0 and not ev[1][3].any() and not ev[2][3].any()  # no view: zeros
    assert not np.isfinite(ev[0][[4, 6]]).any() and np.isfinite(ev[0][good]).all()


def test_max_steps_one_returns_the_start(fx):
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = R.group(fx, "v12")
    out, st = rp.refine_points_arrays(P, obs, mask, xyz0, max_steps=1)
    assert (st["status"] == R.STEP_LIMIT).all() and np.array_equal(out, xyz0)
    assert (st["n_trials"] == 1).all() and (st["n_accepted"] == 0).all() and np.array_equal(st["cost_initial"], st["cost_final"])
    ev = rp.evaluate_points_cost(P, obs, mask, xyz0)
    assert np.allclose(ev[0], st["cost_initial"], rtol=1e-14, atol=0.0)  # the same accumulation, compiled into another kernel
    two, st2 = rp.refine_points_arrays(P, obs, mask, xyz0, max_steps=2)
    assert (st2["n_trials"] == 2).all() and (st2["n_accepted"] <= 1).all() and (st2["cost_final"] <= st2["cost_initial"]).all()
    assert np.array_equal(two[st2["n_accepted"] == 0], xyz0[st2["n_accepted"] == 0]) and (st2["n_accepted"] == 1).any()
    v = R.views_of(mask[4, 0], 12)
    h = P[v, :, :3] @ two[4, 0] + P[v, :, 3]
    err = np.linalg.norm(h[:, :2] / h[:, 2:3] - obs[4, 0][v], axis=1)
    assert np.allclose(st2["view_err"][4, 0][v], err, rtol=1e-12) and np.isnan(st2["view_err"][4, 0][3:8]).all()
