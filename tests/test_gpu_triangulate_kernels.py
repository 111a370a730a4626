"""The triangulation kernel (csrc/triangulate.hip) on the GPU against the float64 restatement of tests/triangulate_ref.py: statuses,
view counts and inlier masks exactly (no case has a view within 1e-6 px of the threshold: tests/test_triangulate_cpu.py), the points
against a 40-digit evaluation of the same final system with numpy's own error as the yardstick, the errors at the GPU's own point,
the undistortion recurrence, and non-finite problems beside finite neighbours."""
import numpy as np
import pytest

import triangulate_cases as cases
import triangulate_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -45


def gpu(P, obs, scores=None, **kw):
    from smilify_amd import triangulate

    return triangulate.triangulate_arrays(P, obs, scores, **kw)


def check_structure(out, res, P, thr):
    assert np.array_equal(out["status"], R.field(res, "status"))
    assert np.array_equal(out["views_used"], R.field(res, "views_used"))
    assert np.array_equal(out["inlier_mask"], R.field(res, "cam_mask", np.uint32))
    for idx in np.ndindex(res.shape):
        r, X = res[idx], out["xyz"][idx]
        if r["status"] != 0:
            assert np.isnan(X).all() and np.isnan(out["mean_err"][idx]) and np.isnan(out["view_err"][idx]).all()
            continue
        v = r["valid"]
        e = R.reproj_errors(P[v], X, r["pts"][v])  # the restatement's errors at the GPU's own point
        assert np.isnan(out["view_err"][idx][~v]).all()
        assert np.allclose(out["view_err"][idx][v], e, rtol=1e-9, atol=1e-9)
        assert np.isclose(out["mean_err"][idx], e.mean(), rtol=1e-9, atol=1e-9)
        assert R.rel_err(X, r["xyz"]) < 1e-6  # (the accuracy test below measures this properly)


@pytest.mark.parametrize("name", cases.CASES)
def test_structure_of_generated_cases(name):
    c = cases.get(name)
    out = gpu(c["P"], c["obs"], min_views=c["min_views"], reproj_threshold=c["thr"], use_ransac=c["use_ransac"])
    check_structure(out, c["res"], c["P"], c["thr"])


def test_lowest_index_hypothesis_wins_a_tie():
    """Two hypotheses count the same number of inliers and disagree on which: the winner is seen through the inlier mask."""
    c = cases.get("ties")
    out = gpu(c["P"], c["obs"], reproj_threshold=c["thr"])
    for i, r in enumerate(c["res"].ravel()):
        top = np.flatnonzero(r["hyp_count"] == r["hyp_count"].max())
        last = sum(1 << int(k) for k in np.flatnonzero(r["hyp_err"][top[-1]] < c["thr"]))  # what a "last maximum" reduction would keep
        assert r["cam_mask"] != last
        assert int(out["inlier_mask"][i, 0]) == r["cam_mask"], (i, top)


@pytest.mark.parametrize("ncam,use_ransac,mv", [(n, u, m) for n in (12, 5) for u in (True, False) for m in (2, 3)])
def test_structure_of_the_reference_fixture(ncam, use_ransac, mv):
    fx = R.fixture()
    P, obs, scores = R.fixture_arrays(fx, ncam)
    res = R.solve_all(P, obs, scores, conf=0.3, min_views=mv, thr=15.0, use_ransac=use_ransac)
    out = gpu(P, obs, scores, confidence_threshold=0.3, min_views=mv, reproj_threshold=15.0, use_ransac=use_ransac)
    check_structure(out, res, P, 15.0)
    assert np.array_equal(np.isnan(out["obs_undistorted"]).any(axis=-1), ~R.field(res, "valid"))


def test_a_batch_over_many_workgroups_repeats_its_problems():
    c = cases.get("n4")
    reps = 101  # 505 problems: 127 workgroups, the last with one problem
    one = gpu(c["P"], c["obs"])
    many = gpu(c["P"], np.tile(c["obs"], (reps, 1, 1, 1)))
    for k in ("xyz", "status", "views_used", "mean_err", "view_err", "inlier_mask"):
        assert np.array_equal(many[k], np.tile(one[k], (reps,) + (1,) * (one[k].ndim - 1)), equal_nan=True), k


@pytest.mark.parametrize("name", cases.ACCURACY_SETS)
def test_accuracy_against_forty_digits(name):
    """max |X_gpu - X_mp| / |X_mp| <= 4 x max |X_numpy - X_mp| / |X_mp| over the set, both against the 40-digit solution of the same
    final system, with a floor of 2^-45 where numpy is exact to the last bits."""
    c = cases.get(name)
    out = gpu(c["P"], c["obs"], min_views=c["min_views"], reproj_threshold=c["thr"], use_ransac=c["use_ransac"])
    e_gpu = e_np = 0.0
    for idx in np.ndindex(c["res"].shape):
        r = c["res"][idx]
        if r["status"] != 0:
            continue
        assert int(out["inlier_mask"][idx]) == r["cam_mask"]  # the same final system
        X_mp = R.dlt_mp(R.final_system(c["P"], r))
        e_gpu, e_np = max(e_gpu, R.rel_err(out["xyz"][idx], X_mp)), max(e_np, R.rel_err(r["xyz"], X_mp))
    print(f"accuracy {name}: gpu {e_gpu:.3e} numpy {e_np:.3e} bound {max(4.0 * e_np, FLOOR):.3e}")
    assert e_gpu <= max(4.0 * e_np, FLOOR), (e_gpu, e_np)


def test_undistortion():
    """The five-round recurrence in the kernel's load phase against the restatement's, on 2 cameras x 16 points; a camera with
    all-zero coefficients is bit-identical to a call without undistortion."""
    P = R.ring_rig(2, 8)
    obs, _ = R.make_cases(P, 16, 9, outliers=0)
    K = np.stack([np.array([[1100.0, 0.0, 640.0], [0.0, 1110.0, 512.0], [0.0, 0.0, 1.0]]), np.array([[950.0, 0.5, 600.0], [0.0, 960.0, 500.0], [0.0, 0.0, 1.0]])])
    dist = np.array([[-0.35, 0.12, 2e-3, -1.5e-3, -0.02], [0.25, -0.08, -1e-3, 2e-3, 0.01]])  # strong: the points lie near the centre
    out = gpu(P, obs, K=K, dist=dist, use_ransac=False)
    for c in range(2):
        ref = R.undistort5(obs[:, 0, c], K[c], dist[c])
        assert np.abs(ref - obs[:, 0, c]).max() > 0.5  # the distortion moves the points
        assert (np.abs(out["obs_undistorted"][:, 0, c] - ref) <= 1e-12 * np.abs(ref)).all()
    res = R.solve_all(P, obs, None, use_ransac=False, K=K, dist=dist)
    assert np.array_equal(out["status"], R.field(res, "status")) and np.abs(out["xyz"] - R.field(res, "xyz")).max() < 1e-9
    plain = gpu(P, obs, use_ransac=False)
    half = gpu(P, obs, K=K, dist=np.stack([np.zeros(5), dist[1]]), use_ransac=False)
    zero = gpu(P, obs, K=K, dist=np.zeros((2, 5)), use_ransac=False)
    assert np.array_equal(half["obs_undistorted"][:, :, 0], obs[:, :, 0]) and np.array_equal(half["obs_undistorted"][:, :, 1], out["obs_undistorted"][:, :, 1])
    for k in plain:
        assert np.array_equal(plain[k], zero[k], equal_nan=True), k
    from smilify_amd import triangulate

    und = triangulate.undistort_points(obs[:, 0, 0], K[0], dist[0])  # the public function: the same load phase
    assert np.array_equal(und, out["obs_undistorted"][:, 0, 0])


def test_non_finite_problems_leave_their_neighbours_alone():
    """Two parallel rays (X[3] = 0 in exact arithmetic: the point is at infinity) and a NaN score, between ordinary problems: the
    kernel runs to completion, gives the reference's outcome (status 0 from two views; whatever IEEE division makes of X[:3] / X[3]),
    and the neighbours come out as they do alone.  The VALUE of the point at infinity is deliberately not compared: it is a rounding
    error of 1e-17 divided into 0.6 in numpy and here alike, and only "not finite, or beyond 1e12" can be asked of either."""
    P2 = np.stack([np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([np.eye(3), np.array([[1.0], [0.0], [0.0]])])])
    c = cases.get("n4")
    P = np.concatenate([P2, c["P"][:2]])  # cameras 0, 1: the parallel pair; 2, 3: two of the ring
    good = np.full((1, 1, 4, 2), np.nan)
    good[0, 0, 2:] = c["obs"][0, 0, :2]
    par = np.full((1, 1, 4, 2), np.nan)
    par[0, 0, :2] = [[1.0, 1.0], [1.0, 1.0]]  # the ray (1, 1, 1) from both centres
    obs = np.concatenate([good, par, good, good, good])
    scores = np.full((5, 1, 4), 0.9)
    scores[3, 0, 2] = np.nan  # an unknown score keeps its view
    scores[4, 0, 2] = 0.1     # a low one drops it: one view left
    out = gpu(P, obs, scores, use_ransac=True)
    res = R.solve_all(P, obs, scores, use_ransac=True)
    assert out["status"].ravel().tolist() == R.field(res, "status").ravel().tolist() == [0, 0, 0, 0, 1]
    assert out["views_used"].ravel().tolist() == [2, 2, 2, 2, 0]
    far = out["xyz"][1, 0]
    assert not np.isfinite(far).all() or np.abs(far).max() > 1e12  # at infinity, as far as float64 can say
    ref_far = res[1, 0]["xyz"]
    assert not np.isfinite(ref_far).all() or np.abs(ref_far).max() > 1e12
    alone = gpu(P, good, use_ransac=True)
    for i in (0, 2, 3):
        assert np.array_equal(out["xyz"][i], alone["xyz"][0]) and out["mean_err"][i, 0] == alone["mean_err"][0, 0]
    assert np.isnan(out["xyz"][4]).all()
