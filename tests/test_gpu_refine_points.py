"""The point refinement on the GPU (smilify_amd.refine_points on csrc/refine_points.hip) against scipy's runs
(tests/golden/refine_points_ref.npz) and the numpy restatement of the kernel's Levenberg-Marquardt (tests/refine_points_ref.py), and the
Python layer on top of it: triangulate_all(refine=True) and the alternating bundle adjustment.

Bounds.  Cost: final <= initial exactly (the accept rule), final <= scipy-default's (1 + 1e-9) (scipy stops at ftol = 1e-8 above the
minimum) and >= scipy-tight's (1 - 1e-9): the bounds of the camera refinement, for the same stopping rule.  Points: against the TIGHT
solution within max(4 x the restatement's own distance to it, POINT_FLOOR), relative to |X|.  POINT_FLOOR = 1e-6: the iteration ends
when an accepted step lowers the cost by less than 1e-12 of it and a cost is quadratic in the distance to its minimum, so the rule
fixes the point to the square root, 1e-6, and no further.  Every problem of the committed file is run; none is left out.

Trial counts are printed next to the restatement's and NOT asserted equal: the CPU run (test_refine_points_cpu.py) shows accept
decisions of the fixture with a relative cost margin of 7e-16, far below 1e-10, so a last-bit difference of the sums may flip one."""
import numpy as np
import pytest

import refine_points_ref as R
import refine_ref as RC
import triangulate_ref as T

pytestmark = pytest.mark.gpu
POINT_FLOOR = 1e-6


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def runs(fx):
    """refine_points_arrays on every group of the fixture: once."""
    from smilify_amd import refine_points as rp

    return {g: rp.refine_points_arrays(*R.group(fx, g), f_scale=float(fx["f_scale"])) for g in R.GROUPS}


@pytest.mark.parametrize("g", R.GROUPS)
def test_fits_against_scipy(fx, runs, g):
    xyz, st = runs[g]
    ref = R.lm_group(fx, g)
    assert xyz.shape == fx[g + "_xyz0"].shape and set(st) == {"status", "n_accepted", "n_trials", "cost_initial", "cost_final", "view_err"}
    for i, r in enumerate(ref):
        tight, cost = fx[g + "_tight_x"][i], st["cost_final"][i, 0]
        d_gpu, d_ref = R.distance(xyz[i, 0], tight), R.distance(r["xyz"], tight)
        print(f"{g} {i}: status {st['status'][i, 0]} trials {st['n_trials'][i, 0]} (restatement {r['n_trials']}) accepted {st['n_accepted'][i, 0]} "
              f"cost/scipy - 1 {cost / fx[g + '_scipy_cost'][i] - 1:.2e} cost/tight - 1 {cost / fx[g + '_tight_cost'][i] - 1:.2e} "
              f"distance to tight: gpu {d_gpu:.2e} restatement {d_ref:.2e}")
        assert st["status"][i, 0] in (R.CONVERGED, R.STEP_LIMIT) and st["status"][i, 0] == r["status"]
        assert 1 <= st["n_accepted"][i, 0] + 1 <= st["n_trials"][i, 0] <= 50
        assert cost <= st["cost_initial"][i, 0]  # exactly
        assert st["cost_initial"][i, 0] == pytest.approx(r["cost0"], rel=1e-12)
        assert cost / fx[g + "_scipy_cost"][i] - 1.0 <= 1e-9
        assert cost / fx[g + "_tight_cost"][i] - 1.0 >= -1e-9
        assert d_gpu <= max(4.0 * d_ref, POINT_FLOOR), (g, i, d_gpu, d_ref)


def test_the_outlier_cases_end_nearer_the_truth_than_their_dlt_start(fx, runs):
    """One 10 - 14 px outlier inside the mask (3, 12 and 32 views).  A plain least-squares weight does not achieve this in the 12-view
    case: its minimum is farther from the truth than the DLT start (test_refine_points_cpu.py prints the three distances)."""
    for g in (str(s) for s in fx["outlier_cases"]):
        truth = fx[g + "_X_true"][0]
        d0, d1 = np.linalg.norm(fx[g + "_xyz0"][0, 0] - truth), np.linalg.norm(runs[g][0][0, 0] - truth)
        print(f"outlier case {g}: |X - true| DLT {d0:.3e} refined {d1:.3e}")
        assert d1 < d0, g


def test_triangulate_all_with_refinement():
    """The 12-camera triangulation fixture: statuses, views and masks as without the refinement, every refined problem's soft_l1 cost
    at or below its DLT point's, the errors those of the refined points."""
    from smilify_amd import refine_points as rp
    from smilify_amd import triangulate as tri

    fx_t = T.fixture()
    P, obs, scores = T.fixture_arrays(fx_t, 12)
    K, dist = fx_t["K"], np.zeros((12, 5))
    plain = tri.triangulate_arrays(P, obs, scores, K, dist, 0.3, 2, 15.0, True)
    fine = tri.triangulate_arrays(P, obs, scores, K, dist, 0.3, 2, 15.0, True, refine=True)
    for k in ("status", "views_used", "inlier_mask"):
        assert np.array_equal(plain[k], fine[k]), k
    assert np.array_equal(plain["obs_undistorted"], fine["obs_undistorted"], equal_nan=True)
    ok = plain["status"] == 0
    assert ok.sum() == 45 and np.isnan(fine["xyz"][~ok]).all() and (fine["refine_status"][~ok] == R.FEW_VIEWS).all()  # a failed problem has no view in its mask
    assert (fine["refine_status"][ok] <= R.STEP_LIMIT).all()
    assert (fine["refine_cost_final"][ok] <= fine["refine_cost_initial"][ok]).all() and (fine["xyz"][ok] != plain["xyz"][ok]).any(axis=-1).all()
    host = rp.observation_costs(P, fine["obs_undistorted"], fine["inlier_mask"], fine["xyz"]).sum(axis=(2, 3))
    host0 = rp.observation_costs(P, plain["obs_undistorted"], plain["inlier_mask"], plain["xyz"]).sum(axis=(2, 3))
    assert np.allclose(host[ok], fine["refine_cost_final"][ok], rtol=1e-12) and np.allclose(host0[ok], fine["refine_cost_initial"][ok], rtol=1e-12)
    assert (host[ok] <= host0[ok]).all()
    f, k = np.argwhere(ok)[5]
    valid = ~np.isnan(fine["obs_undistorted"][f, k]).any(axis=-1)
    err = T.reproj_errors(P[valid], fine["xyz"][f, k], fine["obs_undistorted"][f, k][valid])
    assert np.allclose(fine["view_err"][f, k][valid], err, rtol=1e-12) and np.isnan(fine["view_err"][f, k][~valid]).all()
    assert fine["mean_err"][f, k] == pytest.approx(err.mean(), rel=1e-12) and valid.sum() >= fine["views_used"][f, k]
    assert np.array_equal(np.isnan(plain["view_err"]), np.isnan(fine["view_err"]))

    cams, coords, sc = T.fixture_calibration(fx_t, 12)
    tracks0, stats0 = tri.triangulate_all(cams, coords, sc, 6, 8, min_views=2, verbose=False)
    tracks, stats = tri.triangulate_all(cams, coords, sc, 6, 8, min_views=2, verbose=False, refine=True)
    assert np.array_equal(tracks0[:, 0], np.where(ok[..., None], plain["xyz"], np.nan), equal_nan=True)
    assert np.array_equal(tracks[:, 0], np.where(ok[..., None], fine["xyz"], np.nan), equal_nan=True)
    assert stats["refined"] == 45 and set(stats) == set(stats0) | {"refined"}
    for key in ("triangulated", "failed_insufficient_views", "failed_ransac", "mean_views_used"):
        assert stats[key] == stats0[key]
    assert stats["mean_reproj_error_px"] == pytest.approx(float(fine["mean_err"][ok].mean()), rel=1e-12)


def test_bundle_adjust_alternating_descends():
    """The 12-camera, 40 x 8 scene of the camera refinement fixture from its perturbed cameras: the total never rises over the six half
    steps, and the point kernel's total equals the camera kernel's on every state."""
    from smilify_amd import refine_points as rp
    from smilify_amd import triangulate as tri

    fx_c = RC.fixture()
    names = RC.names(fx_c)
    cams = {n: RC.camera_of(fx_c["init_params"][c]) for c, n in enumerate(names)}
    P = np.stack([tri.get_projection_matrix(cams[n]) for n in names])
    obs = np.ascontiguousarray(fx_c["scene_coords"].transpose(1, 2, 0, 3))
    scores = np.ascontiguousarray(fx_c["scene_scores"].transpose(1, 2, 0))
    start = tri.triangulate_arrays(P, obs, scores, None, None, 0.3, 3, 15.0, True)
    assert (start["status"] == 0).sum() > 300
    refined, xyz, history = rp.bundle_adjust_alternating(cams, start["obs_undistorted"], start["inlier_mask"], start["xyz"], iterations=3)
    assert [h["half"] for h in history] == ["start"] + ["points", "cameras"] * 3 and [h["iteration"] for h in history] == [0, 1, 1, 2, 2, 3, 3]
    print("bundle adjustment totals:", [(h["half"], round(h["total"], 6), f"{h['total_by_camera'] / h['total'] - 1:.1e}") for h in history])
    for prev, h in zip(history, history[1:]):
        assert h["total"] <= prev["total"] * (1.0 + 1e-12), (prev, h)
    for h in history:
        assert np.isfinite(h["total"]) and abs(h["total_by_camera"] - h["total"]) <= 1e-12 * h["total"], h
    assert history[-1]["total"] < 0.5 * history[0]["total"]  # the cameras start 0.01 rad and 2 cm off
    assert all(h["held_fixed"] == [] for h in history if h["half"] == "cameras")
    assert sorted(refined) == names and xyz.shape == start["xyz"].shape
    ok = start["status"] == 0
    assert np.array_equal(np.isnan(xyz), np.isnan(start["xyz"])) and (xyz[ok] != start["xyz"][ok]).any()
    assert "rvec" in refined[names[0]] and not np.array_equal(refined[names[0]]["K"], cams[names[0]]["K"])

    # a camera that sees fewer than 20 points is held fixed, and the result says so
    few = start["inlier_mask"].copy()
    seen = np.cumsum((few >> np.uint32(11)) & np.uint32(1)).reshape(few.shape)
    few[seen > 19] &= np.uint32(~(1 << 11) & 0xFFFFFFFF)
    held, _, hist = rp.bundle_adjust_alternating(cams, start["obs_undistorted"], few, start["xyz"], iterations=1)
    assert hist[-1]["held_fixed"] == [names[11]] and hist[-1]["cameras"][names[11]]["status"] == "skipped"
    assert np.array_equal(held[names[11]]["K"], cams[names[11]]["K"]) and np.array_equal(held[names[11]]["t"], cams[names[11]]["t"])
    assert hist[2]["total"] <= hist[1]["total"] * (1.0 + 1e-12) <= hist[0]["total"] * (1.0 + 1e-12) ** 2
