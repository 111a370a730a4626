"""The camera refinement without a GPU: the ABI's argument checks, the restatement (tests/refine_ref.py) against the reference's own
run (tests/golden/refine_cameras_ref.npz) under the acceptance rules of the GPU tests, Rodrigues and its derivative against central
differences, and gather_correspondences / quick_reproj_stats / the packing against the reference's recorded outputs."""
import ctypes
import os

import numpy as np
import pytest

import refine_ref as R

PARAM_FLOOR = 1e-6  # see test_gpu_refine.py


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def test_argument_checks_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(R.GOLDEN)), "include", "smilfit.h")).read()
    assert "#define SMIL_REFINE_MIN_POINTS 20" in header and _lib.REFINE_MIN_POINTS == R.MIN_POINTS == 20
    err = lambda: lib.smil_last_error()  # noqa: E731
    one = ctypes.c_void_p(256)  # never dereferenced: every call below fails before a launch
    good = np.array([0, 30, 30, 75], np.int64)

    def call(fn="cameras", C=3, offsets=good, n_params=10, f_scale=5.0, max_steps=10, pts=one, params=one, out=one, ws=one, off_dev=one):
        off = None if offsets is None else offsets.ctypes.data_as(ctypes.c_void_p)
        if fn == "evaluate":
            return lib.smil_refine_evaluate(pts, pts, off, off_dev, C, params, n_params, f_scale, out, out, out, ws, None)
        return lib.smil_refine_cameras(pts, pts, off, off_dev, C, params, n_params, f_scale, max_steps, out, out, out, out, out, out, out,
                                       ws, None)

    for fn in ("cameras", "evaluate"):
        assert call(fn, C=0) == -1 and b"C=0" in err()
        assert call(fn, n_params=7) == -1 and b"n_params=7" in err()
        assert call(fn, f_scale=0.0) == -1 and b"f_scale" in err()
        assert call(fn, f_scale=-1.0) == -1 and b"f_scale" in err()
        assert call(fn, f_scale=float("nan")) == -1 and b"f_scale" in err()
        assert call(fn, offsets=None) == -1 and b"null" in err()
        assert call(fn, ws=None) == -1 and b"null" in err()
        assert call(fn, offsets=np.array([1, 30, 30, 75], np.int64)) == -1 and b"offsets[0]" in err()
        assert call(fn, offsets=np.array([0, 30, 29, 75], np.int64)) == -1 and b"monotone" in err() and b"camera 1" in err()
        assert call(fn, pts=None) == -1 and b"null" in err()
        assert call(fn, params=None) == -1 and b"null" in err()
        assert call(fn, out=None) == -1 and b"null" in err()
        assert call(fn, off_dev=None) == -1 and b"null" in err()
    assert call(max_steps=0) == -1 and b"max_steps=0" in err()
    assert lib.smil_refine_workspace_bytes(0, 10) == 0 and lib.smil_refine_workspace_bytes(3, -1) == 0
    small, large = lib.smil_refine_workspace_bytes(3, 256), lib.smil_refine_workspace_bytes(3, 257)
    assert 0 < small < large  # a second workgroup per camera: a second partial
    assert lib.smil_refine_workspace_bytes(3, 10 ** 9) == lib.smil_refine_workspace_bytes(3, 64 * 256)  # the cap of the grid


def test_python_checks_without_gpu():
    import torch

    from smilify_amd import _lib, engine

    t = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(_lib.SmilError, match="GPU"):
        engine.refine_evaluate(t, t[:, :2], np.array([0, 5]), torch.zeros(1, 10, dtype=torch.float64))
    with pytest.raises(ValueError, match="max_steps"):
        engine.refine_cameras(t, t[:, :2], np.array([0, 5]), torch.zeros(1, 10, dtype=torch.float64), max_steps=0)
    with pytest.raises(ValueError, match="offsets"):
        engine.refine_cameras(t, t[:, :2], np.array([0, 5, 4]), torch.zeros(2, 10, dtype=torch.float64))


@pytest.mark.parametrize("n_params", [10, 6])
def test_restatement_reproduces_the_reference(fx, n_params):
    """Statuses equal; the cost ends at or below scipy's (scipy stops at ftol = 1e-8) and not below the tight solution's; R, t, K
    within the floor of the tight solution."""
    tight = R.tight10(fx, n_params)
    for c, (p3, p2) in enumerate(R.correspondences(fx)):
        r = R.lm(fx["init_params"][c], p3, p2, n_params, float(fx["f_scale"]))
        if fx[f"p{n_params}_status"][c] == "skipped":
            assert r["status"] == R.SKIPPED and len(p3) == 19 and np.array_equal(r["params"], fx["init_params"][c])
            continue
        assert r["status"] == R.CONVERGED and fx[f"p{n_params}_status"][c] == "success"
        assert 2 <= r["n_accepted"] + 1 <= r["n_trials"] <= 100
        assert r["cost"] <= fx[f"p{n_params}_scipy_cost"][c] * (1.0 + 1e-9) and r["cost"] < r["cost0"]
        assert r["cost"] >= fx[f"p{n_params}_tight_cost"][c] * (1.0 - 1e-9)
        d = R.rotation_distance(r["params"], tight[c])
        print(f"restatement p{n_params} cam {c}: trials {r['n_trials']} cost/scipy - 1 {r['cost'] / fx[f'p{n_params}_scipy_cost'][c] - 1:.2e} "
              f"distance to tight R {d[0]:.2e} t {d[1]:.2e} K {d[2]:.2e}")
        assert max(d) <= PARAM_FLOOR
        if n_params == 6:
            assert np.array_equal(r["params"][6:], fx["init_params"][c][6:])
    assert len(fx["counts"]) == 12 and {19, 20, 255, 256, 257, 549} <= set(fx["counts"].tolist())
    assert not fx["init_params"][int(fx["zero_cam"]), :3].any()  # rvec = 0 exactly


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1e-4, 1.0, 3.1])
def test_rodrigues_and_its_derivative(theta):
    """R is a rotation by theta about the axis, and dR matches central differences of R (step 1e-6: truncation ~1e-12, rounding
    ~1e-10).  theta = 0: R = I exactly and the derivative is the generators.  The product's own numpy Rodrigues gives the same R."""
    from smilify_amd import refine_cameras as rc

    axis = np.array([0.36, -0.48, 0.8])
    r = theta * axis
    Rm, dR = R.rodrigues(r)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(Rm) - 1.0) < 1e-15
    assert abs(np.trace(Rm) - (1.0 + 2.0 * np.cos(theta))) < 4e-16 and (theta == 0.0 or np.abs(Rm @ axis - axis).max() < 4e-16)
    assert np.abs(rc.rodrigues(r) - Rm).max() < 4e-16
    if theta == 0.0:
        assert np.array_equal(Rm, np.eye(3)) and np.array_equal(dR, R.GEN) and np.array_equal(rc.rodrigues(r), np.eye(3))
    h = 1e-6
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num = (R.rodrigues(r + e)[0] - R.rodrigues(r - e)[0]) / (2.0 * h)
        assert np.abs(num - dR[k]).max() < 1e-9, (theta, k)
    if theta in (1.0, 3.1):
        assert np.abs(rc.rotation_to_rvec(Rm) - r).max() < 1e-12 * max(1.0, 1.0 / np.sin(theta))


def test_jacobian_against_central_differences(fx):
    p3, p2 = R.correspondences(fx)[8]
    x = fx["init_params"][8]
    _, Ju, Jv = R.jacobian(x, p3)
    for k in range(10):
        h = 1e-6 * max(1.0, abs(x[k]))
        e = np.zeros(10)
        e[k] = h
        num = (R.jacobian(x + e, p3)[0] - R.jacobian(x - e, p3)[0]) / (2.0 * h)
        scale = max(np.abs(Ju[:, k]).max(), np.abs(Jv[:, k]).max())
        assert np.abs(num[:, 0] - Ju[:, k]).max() < 1e-7 * scale and np.abs(num[:, 1] - Jv[:, k]).max() < 1e-7 * scale, k
    cost, g, H = R.evaluate(x, p3, p2)
    cost_mp, g_mp, H_mp = R.evaluate_mp(x, p3, p2)
    assert abs(cost / cost_mp - 1.0) < 1e-13 and R.rel_err(g, g_mp) < 1e-13 and R.rel_err(H, H_mp) < 1e-13


def test_gather_pack_and_stats_equal_the_reference(fx):
    from smilify_amd import refine_cameras as rc

    tracks, coords, scores = fx["scene_tracks"], fx["scene_coords"], fx["scene_scores"]
    kp_3d = tracks[:, 0]
    valid_3d = ~np.isnan(kp_3d).any(axis=-1) & (kp_3d != 0).any(axis=-1)
    cams = {n: R.camera_of(fx["init_params"][c]) for c, n in enumerate(R.names(fx))}
    drawn = []

    class Spy:
        def __init__(self, seed):
            self.g = np.random.default_rng(seed)

        def choice(self, *a, **kw):
            r = self.g.choice(*a, **kw)
            drawn.append(np.asarray(r))
            return r

    spy, g3, g2 = Spy(43), [], []
    for c, n in enumerate(R.names(fx)[:3]):
        p3, p2 = rc.gather_correspondences(kp_3d, valid_3d, coords[c], scores[c], cams[n], 0.3, max_points=150, rng=spy)
        g3.append(p3), g2.append(p2)
    assert [len(p) for p in g3] == fx["gather_n"].tolist() == [150] * 3
    assert np.array_equal(np.stack(drawn), fx["gather_draws"])  # the caller's generator, drawn from as the reference draws
    assert np.array_equal(np.concatenate(g3), fx["gather_pts_3d"]) and np.array_equal(np.concatenate(g2), fx["gather_pts_2d"])
    p3, p2 = rc.gather_correspondences(kp_3d, valid_3d, coords[5], scores[5], cams["cam05"], 0.3)  # the mask alone
    assert np.array_equal(p3, fx["gather_full_pts_3d"]) and np.array_equal(p2, fx["gather_full_pts_2d"]) and 150 < len(p3) < 320
    empty = rc.gather_correspondences(kp_3d, np.zeros_like(valid_3d), coords[5], scores[5], cams["cam05"], 0.3)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 2)

    q = rc.quick_reproj_stats(tracks, {n: coords[c] for c, n in enumerate(R.names(fx))}, {n: scores[c] for c, n in enumerate(R.names(fx))},
                              cams, 0.3, max_points_per_cam=200)
    assert list(q) == fx["quick_keys"].tolist()
    assert np.allclose([float(q[k]) for k in fx["quick_keys"]], fx["quick_stats"], rtol=1e-9, atol=0)

    for intr, n in ((True, 10), (False, 6)):
        x = rc.pack_params(cams["cam03"], intr)
        assert np.array_equal(x, fx["init_params"][3][:n])
        cam = rc.unpack_params(fx[f"p{n}_scipy_x"][3], cams["cam03"], intr)
        assert np.array_equal(rc.pack_params(cam, intr), fx[f"p{n}_scipy_x"][3]) and cams["cam03"]["t"].shape == cam["t"].shape == (3, 1)
        if not intr:
            assert np.array_equal(cam["K"], cams["cam03"]["K"])
        res = rc.reprojection_residuals(x, *R.correspondences(fx)[3], cams["cam03"], intr)
        err = np.sqrt(res[::2] ** 2 + res[1::2] ** 2)
        stats = dict(zip(fx["stat_keys"], fx[f"p{n}_stats"][3]))
        assert np.median(err) == pytest.approx(stats["median_err_before"], rel=1e-9)
        assert 100 * (err < 5).mean() == pytest.approx(stats["pct_under_5px_before"], rel=1e-12)
    no_rvec = {k: v for k, v in cams["cam03"].items() if k != "rvec"}  # a calibration of triangulate_all: R and no rvec
    assert np.abs(rc.rodrigues(rc.pack_params(no_rvec)[:3]) - cams["cam03"]["R"]).max() < 1e-15
