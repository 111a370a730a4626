"""The point refinement without a GPU: the ABI's argument checks, the restatement (tests/refine_points_ref.py) against scipy's runs
(tests/golden/refine_points_ref.npz) under the acceptance rules of the GPU tests, the fixture's ambiguity condition, the Jacobian against
central differences, the masking, the two ways of summing the total cost, and triangulate_all's unchanged default."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import refine_points_ref as R
import triangulate_ref as T

POINT_FLOOR = 1e-6  # see test_gpu_refine_points.py
SAME = 1e-5         # the fixture's ambiguity condition


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def test_argument_checks_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(R.GOLDEN)), "include", "smilfit.h")).read()
    assert "#define SMIL_REFINE_POINTS_FEW_VIEWS 2" in header and _lib.REFINE_POINTS_FEW_VIEWS == R.FEW_VIEWS == 2
    assert (_lib.REFINE_CONVERGED, _lib.REFINE_STEP_LIMIT, _lib.REFINE_NONFINITE) == (R.CONVERGED, R.STEP_LIMIT, R.NONFINITE)
    assert b"0.3" in lib.smil_version()  # the layout number stays
    err = lambda: lib.smil_last_error()  # noqa: E731
    one = ctypes.c_void_p(256)  # never dereferenced: every call below fails, or has nothing to do, before a launch

    def call(fn="points", N=3, Kp=2, C=4, f_scale=5.0, max_steps=10, P=one, obs=one, mask=one, xyz=one, out=one, view_err=None):
        if fn == "evaluate":
            return lib.smil_refine_points_evaluate(P, obs, mask, xyz, N, Kp, C, f_scale, out, out, out, None)
        return lib.smil_refine_points(P, obs, mask, xyz, N, Kp, C, f_scale, max_steps, out, out, out, out, out, out, view_err, None)

    for fn in ("points", "evaluate"):
        assert call(fn, C=0) == -1 and b"C=0" in err()
        assert call(fn, C=-1) == -1 and b"C=-1" in err()
        assert call(fn, C=33) == -3 and b"C=33" in err() and b"SMIL_TRI_MAX_VIEWS" in err()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(fn, f_scale=bad) == -1 and b"f_scale" in err()
        assert call(fn, N=-1) == -1 and b"N=-1" in err()
        assert call(fn, Kp=-1) == -1 and b"Kp=-1" in err()
        assert call(fn, N=2 ** 40, Kp=2 ** 20) == -1 and b"exceed the grid" in err()
        for name in ("P", "obs", "mask", "xyz", "out"):
            assert call(fn, **{name: None}) == -1 and b"null" in err(), name
        assert call(fn, N=0) == 0 and call(fn, Kp=0) == 0 and call(fn, N=0, Kp=0, P=None, obs=None, out=None) == 0  # nothing to do
        assert call(fn, N=0, C=0) == -1 and call(fn, N=0, f_scale=0.0) == -1  # checked all the same
    assert call(max_steps=0) == -1 and b"max_steps=0" in err()
    assert call(N=0, max_steps=0) == -1


def test_python_checks_without_gpu():
    import torch

    from smilify_amd import _lib, engine
    from smilify_amd import refine_points as rp

    obs = torch.zeros(2, 1, 3, 2, dtype=torch.float64)
    P, mask, xyz = torch.zeros(3, 3, 4, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, 3, dtype=torch.float64)
    with pytest.raises(_lib.SmilError, match="GPU"):
        engine.refine_points(P, obs, mask, xyz)
    with pytest.raises(_lib.SmilError, match="GPU"):
        engine.refine_points_evaluate(P, obs, mask, xyz)
    with pytest.raises(ValueError, match="max_steps"):
        engine.refine_points(P, obs, mask, xyz, max_steps=0)
    with pytest.raises(ValueError, match="obs"):
        engine.refine_points(P, obs[..., 0], mask, xyz)
    sig = inspect.signature(rp.refine_points_arrays).parameters
    assert sig["f_scale"].default == 5.0 and sig["max_steps"].default == 50
    assert inspect.signature(rp.bundle_adjust_alternating).parameters["iterations"].default == 5


def test_restatement_against_scipy_and_the_ambiguity_condition(fx):
    """Every problem of the committed file: scipy-default, scipy-tight and the restatement end at the same minimum (1e-5); the
    restatement's cost is never above scipy-default's beyond rounding nor below the tight one's; its point is at the tight one's to the
    floor.  The closest accept / reject decision of any fit decides whether the GPU test may assert equal trial counts."""
    assert int(fx["kept"]) >= 0.95 * int(fx["generated"]) and sum(len(fx[g + "_obs"]) for g in R.GROUPS) == int(fx["kept"])
    margin, trials = np.inf, []
    for g in R.GROUPS:
        for i, r in enumerate(R.lm_group(fx, g)):
            d = (R.distance(fx[g + "_scipy_x"][i], fx[g + "_tight_x"][i]), R.distance(r["xyz"], fx[g + "_tight_x"][i]),
                 R.distance(r["xyz"], fx[g + "_scipy_x"][i]))
            print(f"restatement {g} {i}: status {r['status']} trials {r['n_trials']} margin {r['margin']:.1e} cost/scipy - 1 "
                  f"{r['cost'] / fx[g + '_scipy_cost'][i] - 1:.2e} cost/tight - 1 {r['cost'] / fx[g + '_tight_cost'][i] - 1:.2e} "
                  f"distances default-tight {d[0]:.1e} own-tight {d[1]:.1e} own-default {d[2]:.1e}")
            assert max(d) <= SAME, (g, i, d)
            assert r["status"] in (R.CONVERGED, R.STEP_LIMIT) and 1 <= r["n_accepted"] + 1 <= r["n_trials"] <= 50
            assert r["cost"] <= r["cost0"] and r["cost"] <= fx[g + "_scipy_cost"][i] * (1.0 + 1e-9)
            assert r["cost"] >= fx[g + "_tight_cost"][i] * (1.0 - 1e-9)
            assert d[1] <= POINT_FLOOR or r["status"] == R.STEP_LIMIT, (g, i, d)
            margin = min(margin, r["margin"])
            trials.append(r["n_trials"])
    print(f"closest accept decision of the fixture: relative cost margin {margin:.2e}; trials {min(trials)} - {max(trials)}")
    assert {len(R.views_of(m, 32)) for g in R.GROUPS for m in fx[g + "_mask"][:, 0]} >= {2, 3, 12, 32}


def test_the_outlier_cases_end_nearer_the_truth_than_the_dlt_start(fx):
    """One 10 - 14 px outlier inside the mask.  In v12 (0.2 px noise on the other views) the robust minimum is nearer the true point
    than the DLT start AND than the plain least-squares minimum (f_scale 1e6: every weight 1), which keeps the outlier's full pull."""
    for g in fx["outlier_cases"]:
        P, obs, mask, xyz0 = R.group(fx, str(g))
        r = R.lm_group(fx, str(g))[0]
        d0, d1 = np.linalg.norm(xyz0[0, 0] - fx[str(g) + "_X_true"][0]), np.linalg.norm(r["xyz"] - fx[str(g) + "_X_true"][0])
        plain = R.lm(P, obs[0, 0], mask[0, 0], xyz0[0, 0], f_scale=1e6)
        d2 = np.linalg.norm(plain["xyz"] - fx[str(g) + "_X_true"][0])
        print(f"outlier case {g}: |X - true| DLT {d0:.3e} robust {d1:.3e} plain least squares {d2:.3e}")
        if g == "v12":
            assert d1 < d0 and d1 < d2


def test_jacobian_against_central_differences(fx):
    P, obs, mask, xyz0 = R.group(fx, "v12")
    X = xyz0[1, 0] + np.array([0.03, -0.02, 0.05])  # off the minimum: g is not the small rest of a cancellation
    v = R.views_of(mask[1, 0], 12)
    q, J = R.jacobian(P[v], X)
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1e-6
        num = (R.jacobian(P[v], X + e)[0] - R.jacobian(P[v], X - e)[0]) / 2e-6
        assert np.abs(num - J[:, :, k]).max() < 1e-7 * np.abs(J[:, :, k]).max(), k
    got, exact = R.evaluate(P, obs[1, 0], mask[1, 0], X), R.evaluate_mp(P, obs[1, 0], mask[1, 0], X)
    assert max(R.errors(got, exact)) < 1e-13 and np.array_equal(got[2], got[2].T)
    h = 1e-6  # g is the gradient of the cost
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num = (R.evaluate(P, obs[1, 0], mask[1, 0], X + e)[0] - R.evaluate(P, obs[1, 0], mask[1, 0], X - e)[0]) / (2 * h)
        assert abs(num - got[1][k]) < 1e-6 * np.abs(got[1]).max()


def test_masked_out_observations_do_not_reach_the_sums(fx):
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = R.group(fx, "v12")
    i = 4  # views 3 .. 7 dropped, their observations NaN
    assert np.isnan(obs[i, 0, 3:8]).all() and not (int(mask[i, 0]) >> 3) & 31
    got = R.evaluate(P, obs[i, 0], mask[i, 0], xyz0[i, 0])
    v = R.views_of(mask[i, 0], 12)
    packed = R.evaluate(P[v], obs[i, 0][v], (1 << len(v)) - 1, xyz0[i, 0])
    assert got[0] == packed[0] and np.array_equal(got[1], packed[1]) and np.array_equal(got[2], packed[2]) and np.isfinite(got[0])
    garbage = obs[i, 0].copy()
    garbage[3:8] = 1e300
    assert R.evaluate(P, garbage, mask[i, 0], xyz0[i, 0])[0] == got[0]
    costs = rp.observation_costs(P, obs[i:i + 1], mask[i:i + 1], xyz0[i:i + 1])
    assert costs.shape == (1, 1, 12, 2) and not costs[0, 0, 3:8].any() and np.isfinite(costs).all()
    assert costs.sum() == pytest.approx(got[0], rel=1e-14)
    assert R.evaluate(P, obs[i, 0], 0, xyz0[i, 0])[0] == 0.0 and R.lm(P, obs[i, 0], 1 << 5, xyz0[i, 0])["status"] == R.FEW_VIEWS


def test_total_cost_by_point_equals_total_by_camera(fx):
    """The same terms either way: with an exactly rounded sum (math.fsum) the two totals are the same number."""
    from smilify_amd import refine_points as rp

    P, obs, mask, xyz0 = R.group(fx, "ring12")
    costs = rp.observation_costs(P, obs, mask, xyz0, float(fx["f_scale"]))
    by_point, by_camera = costs.sum(axis=(2, 3)), costs.sum(axis=(0, 1, 3))
    assert math.fsum(costs.sum(axis=3).ravel()) == math.fsum(costs.transpose(2, 0, 1, 3).sum(axis=3).ravel())
    assert abs(by_point.sum() - by_camera.sum()) <= 1e-13 * by_point.sum()
    for i in (0, 7):
        assert by_point[i, 0] == pytest.approx(R.evaluate(P, obs[i, 0], mask[i, 0], xyz0[i, 0])[0], rel=1e-14)
    bits = rp.view_bits(mask, 12)
    assert bits.shape == (len(obs), 1, 12) and [int(b) for b in bits[0, 0]] == [(int(mask[0, 0]) >> c) & 1 for c in range(12)]


def test_triangulate_all_default_is_unchanged(monkeypatch):
    """refine defaults to False, and then triangulate_all is what it was: on the existing fixture, with the kernel stood in for by the
    numpy restatement of tests/triangulate_ref.py, the tracks and stats are the reference's and the refinement is never entered."""
    import torch

    from smilify_amd import engine
    from smilify_amd import refine_points as rp
    from smilify_amd import triangulate as tri

    assert inspect.signature(tri.triangulate_all).parameters["refine"].default is False
    assert inspect.signature(tri.triangulate_arrays).parameters["refine"].default is False
    fx_t = T.fixture()

    def fake_kernel(P, obs, scores, pairs, *, K, dist, confidence_threshold, min_views, reproj_threshold, mode, **kw):
        res = T.solve_all(P.numpy(), obs.numpy(), scores.numpy(), conf=confidence_threshold, min_views=min_views, thr=reproj_threshold,
                          use_ransac=bool(mode & 1), K=K.numpy(), dist=dist.numpy())
        und = np.where(T.field(res, "valid", bool)[..., None], T.field(res, "pts", np.float64), np.nan)
        f = lambda name, dt: torch.from_numpy(T.field(res, name, dt))  # noqa: E731
        return (f("xyz", np.float64), f("status", np.int32), f("views_used", np.int32), f("mean_err", np.float64), f("view_err", np.float64),
                torch.from_numpy(T.field(res, "cam_mask", np.int64).astype(np.uint32).view(np.int32)), torch.from_numpy(und))

    def never(*a, **kw):
        raise AssertionError("the refinement ran with refine=False")

    monkeypatch.setattr(engine, "require_gpu", lambda device: torch.device("cpu"))
    monkeypatch.setattr(engine, "triangulate", fake_kernel)
    monkeypatch.setattr(tri, "_pair_table_on", lambda dev: None)
    monkeypatch.setattr(rp, "refine_points_arrays", never)
    cams, coords, scores = T.fixture_calibration(fx_t, 12)
    for use_ransac, key in ((True, "all_c12_ransac_mv2"), (False, "all_c12_dlt_mv2")):
        tracks, stats = tri.triangulate_all(cams, coords, scores, 6, 8, min_views=2, use_ransac=use_ransac, verbose=False)
        want = fx_t[key + "_tracks"]
        assert np.array_equal(np.isnan(tracks), np.isnan(want)) and np.allclose(tracks, want, rtol=1e-9, atol=1e-12, equal_nan=True)
        assert list(stats) == fx_t["stat_keys"].tolist()  # no key added
        assert np.allclose([float(stats[k]) for k in fx_t["stat_keys"]], fx_t[key + "_stats"], rtol=1e-9)
