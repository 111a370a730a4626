"""The camera refinement on the GPU (smilify_amd.refine_cameras on csrc/refine.hip) against the reference's own run
(tests/golden/refine_cameras_ref.npz) and the numpy restatement of the kernel's Levenberg-Marquardt (tests/refine_ref.py).

Bounds.  Cost: final <= scipy's (1 + 1e-9) (scipy stops at ftol = 1e-8 above the minimum) and >= the tight solution's (1 - 1e-9).
Parameters: R (entries), t and K (relative to their largest entry) against the TIGHT solution within max(4 x the restatement's own
distance to it, PARAM_FLOOR).  PARAM_FLOOR = 1e-6: the iteration ends when an accepted step lowers the cost by less than 1e-12 of
it, a cost is quadratic in the distance to its minimum, so that rule fixes the parameters to the square root, 1e-6, and no further;
the tight solution itself carries the error of scipy's finite-difference Jacobian.  Medians: the same rule against the fixture's."""
import numpy as np
import pytest

import refine_ref as R

pytestmark = pytest.mark.gpu
PARAM_FLOOR = 1e-6


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def runs(fx):
    """optimize_cameras on the fixture's twelve cameras and the restatement on the same, for 10 and 6 parameters: once."""
    from smilify_amd import refine_cameras as rc

    cams = {n: R.camera_of(fx["init_params"][c]) for c, n in enumerate(R.names(fx))}
    cor = dict(zip(R.names(fx), R.correspondences(fx)))
    out = {}
    for n_params in (10, 6):
        refined, stats = rc.optimize_cameras(cams, cor, optimize_intrinsics=n_params == 10, verbose=False)
        ref = [R.lm(fx["init_params"][c], *cor[n], n_params, float(fx["f_scale"])) for c, n in enumerate(R.names(fx))]
        out[n_params] = (cams, refined, stats, ref)
    return out


@pytest.mark.parametrize("n_params", [10, 6])
def test_statuses_costs_and_parameters(fx, runs, n_params):
    from smilify_amd import refine_cameras as rc

    cams, refined, stats, ref = runs[n_params]
    tight = R.tight10(fx, n_params)
    assert sorted(refined) == sorted(stats) == R.names(fx)
    for c, n in enumerate(R.names(fx)):
        st = stats[n]
        assert st["status"] == fx[f"p{n_params}_status"][c] and st["n_points"] == fx["counts"][c]
        if st["status"] == "skipped":
            assert refined[n] is cams[n] and set(st) == {"status", "n_points"} and c == 1
            continue
        assert ref[c]["status"] == R.CONVERGED and 2 <= st["n_accepted"] + 1 <= st["n_evaluations"] <= 100
        x = rc.pack_params(refined[n], True)
        d_gpu, d_ref = R.rotation_distance(x, tight[c]), R.rotation_distance(ref[c]["params"], tight[c])
        print(f"p{n_params} cam {c}: trials {st['n_evaluations']} (restatement {ref[c]['n_trials']}) cost/scipy - 1 "
              f"{st['cost_final'] / fx[f'p{n_params}_scipy_cost'][c] - 1:.2e} cost/tight - 1 {st['cost_final'] / fx[f'p{n_params}_tight_cost'][c] - 1:.2e} "
              f"distance to tight: gpu R {d_gpu[0]:.2e} t {d_gpu[1]:.2e} K {d_gpu[2]:.2e} | restatement R {d_ref[0]:.2e} t {d_ref[1]:.2e} K {d_ref[2]:.2e}")
        assert st["cost_final"] <= fx[f"p{n_params}_scipy_cost"][c] * (1.0 + 1e-9)
        assert st["cost_final"] >= fx[f"p{n_params}_tight_cost"][c] * (1.0 - 1e-9)
        assert st["cost_initial"] == pytest.approx(ref[c]["cost0"], rel=1e-12) and st["cost_final"] < st["cost_initial"]
        for got, own in zip(d_gpu, d_ref):
            assert got <= max(4.0 * own, PARAM_FLOOR), (c, d_gpu, d_ref)
        if n_params == 6:
            assert np.array_equal(refined[n]["K"], cams[n]["K"])
        assert np.array_equal(refined[n]["R"], rc.rodrigues(refined[n]["rvec"])) and refined[n]["t"].shape == (3, 1)
        assert np.abs(st["gradient"]).max() <= 1e-6 * np.abs(R.evaluate(fx["init_params"][c], *R.correspondences(fx)[c], n_params)[1]).max()


@pytest.mark.parametrize("n_params", [10, 6])
def test_stats_keys_and_medians(fx, runs, n_params):
    from smilify_amd import refine_cameras as rc

    cams, refined, stats, ref = runs[n_params]
    keys = set(fx["stat_keys"].tolist()) | {"status"}
    cor = R.correspondences(fx)
    for c, n in enumerate(R.names(fx)):
        if stats[n]["status"] == "skipped":
            continue
        assert keys <= set(stats[n])
        want = dict(zip(fx["stat_keys"], fx[f"p{n_params}_stats"][c]))
        for k in ("median_err_before", "pct_under_5px_before", "pct_under_10px_before"):  # the same parameters: numpy against numpy
            assert stats[n][k] == pytest.approx(want[k], rel=1e-9), (n, k)
        res = rc.reprojection_residuals(ref[c]["params"][:n_params], *cor[c], cams[n], n_params == 10)
        own = abs(np.median(np.sqrt(res[::2] ** 2 + res[1::2] ** 2)) - want["median_err_after"]) / want["median_err_after"]
        got = abs(stats[n]["median_err_after"] - want["median_err_after"]) / want["median_err_after"]
        print(f"p{n_params} cam {c}: median after {stats[n]['median_err_after']:.6f} px, fixture {want['median_err_after']:.6f}; "
              f"relative distance gpu {got:.2e} restatement {own:.2e}")
        assert got <= max(4.0 * own, PARAM_FLOOR), (n, got, own)
        assert stats[n]["median_err_after"] < stats[n]["median_err_before"]


def test_optimize_camera_alone_step_limit_and_non_finite_start(fx):
    from smilify_amd import refine_cameras as rc

    c, n = 6, "cam06"
    cam, (p3, p2) = R.camera_of(fx["init_params"][c]), R.correspondences(fx)[c]
    refined, st = rc.optimize_camera(n, cam, p3, p2, verbose=False)
    assert set(fx["stat_keys"].tolist()) | {"status"} <= set(st) and st["status"] == "success"
    assert st["cost_final"] <= fx["p10_scipy_cost"][c] * (1.0 + 1e-9) and st["cost_final"] >= fx["p10_tight_cost"][c] * (1.0 - 1e-9)
    _, lim = rc.optimize_camera(n, cam, p3, p2, verbose=False, max_steps=3)
    assert lim["status"] == "converged" and lim["n_evaluations"] == 3 and lim["n_accepted"] == 2  # the reference's word for "not success"
    assert st["cost_final"] < lim["cost_final"] < lim["cost_initial"] == st["cost_initial"]
    bad = R.camera_of(fx["init_params"][c])
    bad["t"][2, 0] = np.nan
    same, nf = rc.optimize_camera(n, bad, p3, p2, verbose=False)
    assert same is bad and nf["status"] == "non_finite" and nf["n_evaluations"] == 1
    skipped, sk = rc.optimize_camera(n, cam, p3[:19], p2[:19], verbose=False)
    assert skipped is cam and sk == {"status": "skipped", "n_points": 19}


def test_refine_cameras_on_the_fixture_scene(fx):
    """The alternation: the median reprojection error falls, the convergence break fires, and the cameras are those of calling
    the pieces by hand."""
    from smilify_amd import refine_cameras as rc
    from smilify_amd import triangulate as tri

    names = R.names(fx)
    cams = {n: {k: v for k, v in R.camera_of(fx["init_params"][c]).items() if k != "rvec"} for c, n in enumerate(names)}  # as triangulate_all takes them
    coords = {n: fx["scene_coords"][c] for c, n in enumerate(names)}
    scores = {n: fx["scene_scores"][c] for c, n in enumerate(names)}
    refined, history = rc.refine_cameras(cams, coords, scores, iterations=8)
    assert 2 <= len(history) < 8 and history[-1]["converged"] and not any(h["converged"] for h in history[:-1])
    assert abs(history[-2]["post"]["median_px"] - history[-1]["post"]["median_px"]) < 0.05
    print("refine_cameras medians:", [(round(h["pre"]["median_px"], 4), round(h["post"]["median_px"], 4)) for h in history])
    assert history[0]["post"]["median_px"] < history[0]["pre"]["median_px"] and history[-1]["post"]["median_px"] < history[0]["pre"]["median_px"]
    assert all(s["status"] == "success" for s in history[0]["cameras"].values())
    assert "rvec" not in cams[names[0]] and "rvec" in refined[names[0]]  # the input is not written to

    # the first iteration by hand
    F, Kp = fx["scene_coords"].shape[1:3]
    kw = dict(n_frames=F, n_keypoints=Kp, confidence_threshold=0.3, min_views=3, reproj_threshold=15.0, undistort=True, use_ransac=True,
              verbose=False, frame_indices=np.sort(np.random.default_rng(42).choice(F, F, replace=False)))
    current = dict(cams)
    for iteration in range(1, len(history) + 1):
        tracks, _ = tri.triangulate_all(current, coords, scores, **kw)
        kp_3d = tracks[:, 0]
        valid_3d = ~np.isnan(kp_3d).any(axis=-1) & (kp_3d != 0).any(axis=-1)
        pre = rc.quick_reproj_stats(tracks, coords, scores, current, 0.3, max_points_per_cam=200000)
        assert pre == history[iteration - 1]["pre"]
        rng = np.random.default_rng(42 + iteration)
        cor = {n: rc.gather_correspondences(kp_3d, valid_3d, coords[n], scores[n], current[n], 0.3, max_points=200000, rng=rng) for n in names}
        current, _ = rc.optimize_cameras(current, cor, verbose=False)
    for n in names:
        for k in ("R", "t", "K"):
            assert np.array_equal(current[n][k], refined[n][k]), (n, k)
