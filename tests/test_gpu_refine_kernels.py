"""One accumulation of the refinement kernel (csrc/refine.hip: cost, g, H) on the GPU against the 40-digit evaluation of
tests/refine_ref.py, with numpy's own error as the yardstick: error <= max(4 x numpy's, 2^-45), relative for the cost and in units
of the largest entry for g and H.  The cameras are the fixture's at their INITIAL parameters (far from the minimum: g is large), their
counts the edges of the 256-lane workgroups (19, 20, 255, 256, 257, 549), one with rvec = 0 exactly."""
import numpy as np
import pytest

import refine_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -45
EDGES = (1, 2, 3, 4, 5, 6)  # cameras with 19, 20, 255, 256, 257, 549 correspondences; camera 4 has rvec = 0


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def gpu(fx, cams, n_params, params=None):
    from smilify_amd import refine_cameras as rc

    cor = R.correspondences(fx)
    x = fx["init_params"][list(cams)] if params is None else params
    return rc.evaluate_cost(x, [cor[c] for c in cams], optimize_intrinsics=n_params == 10, f_scale=float(fx["f_scale"]))


def check(fx, cams, out, n_params, label):
    for i, c in enumerate(cams):
        exact, numpy_own = R.high_precision(fx, c)
        e_gpu = R.errors((out[0][i], out[1][i], out[2][i]), exact, n_params)
        e_np = R.errors((numpy_own[0],) + R.block(numpy_own[1], numpy_own[2], n_params), exact, n_params)
        print(f"accuracy {label} p{n_params} cam {c} (M = {fx['counts'][c]}): gpu cost {e_gpu[0]:.2e} g {e_gpu[1]:.2e} H {e_gpu[2]:.2e} | "
              f"numpy cost {e_np[0]:.2e} g {e_np[1]:.2e} H {e_np[2]:.2e}")
        for got, own in zip(e_gpu, e_np):
            assert got <= max(4.0 * own, FLOOR), (label, c, e_gpu, e_np)
        assert np.array_equal(out[2][i], out[2][i].T)
        assert not out[1][i][n_params:].any() and not out[2][i][n_params:].any()


@pytest.mark.parametrize("n_params", [10, 6])
def test_twelve_cameras_in_one_launch(fx, n_params):
    cams = list(range(12))
    out = gpu(fx, cams, n_params)
    check(fx, cams, out, n_params, "C=12")
    again = gpu(fx, cams, n_params)
    for a, b in zip(out, again):
        assert np.array_equal(a, b)  # bit-identical: no atomics, a fixed order of every sum


@pytest.mark.parametrize("n_params", [10, 6])
@pytest.mark.parametrize("cam", EDGES)
def test_one_camera_at_every_edge_count(fx, cam, n_params):
    """C = 1: the launch has as many workgroups as THIS camera needs (1, 1, 1, 1, 2, 3), unlike the launch of all twelve."""
    out = gpu(fx, [cam], n_params)
    check(fx, [cam], out, n_params, "C=1")
    again = gpu(fx, [cam], n_params)
    for a, b in zip(out, again):
        assert np.array_equal(a, b)


def test_an_empty_camera_between_two_others(fx):
    from smilify_amd import refine_cameras as rc

    cor = R.correspondences(fx)
    x = fx["init_params"][[2, 3, 5]]
    out = rc.evaluate_cost(x, [cor[2], (np.zeros((0, 3)), np.zeros((0, 2))), cor[5]])
    assert out[0][1] == 0.0 and not out[1][1].any() and not out[2][1].any()
    check(fx, [2], [o[0:1] for o in out], 10, "beside an empty camera")
    check(fx, [5], [o[2:3] for o in out], 10, "beside an empty camera")


def test_a_point_behind_the_camera_divides_as_ieee_does(fx):
    """z = 0 exactly for one point: the cost of that camera is not finite, its neighbour's is what it is alone."""
    from smilify_amd import refine_cameras as rc

    cor = R.correspondences(fx)
    p3, p2 = cor[2][0].copy(), cor[2][1]
    x = fx["init_params"][2].copy()
    x[:3] = 0.0  # R = I: z = X.z + t.z
    p3[7, 2] = -x[5]
    out = rc.evaluate_cost(np.stack([x, fx["init_params"][5]]), [(p3, p2), cor[5]])
    assert not np.isfinite(out[0][0])
    alone = rc.evaluate_cost(fx["init_params"][5:6], [cor[5]])
    assert out[0][1] == alone[0][0] and np.array_equal(out[1][1], alone[1][0]) and np.array_equal(out[2][1], alone[2][0])
