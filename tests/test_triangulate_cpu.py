"""The triangulation restatement (tests/triangulate_ref.py) against the reference's own run (tests/golden/triangulate_ref.npz), the
hypothesis table, the ambiguity condition of every case set the GPU tests use, the ABI's argument checks and the undistortion
recurrence.  No GPU."""
import itertools
import os

import numpy as np
import pytest

import triangulate_cases as cases
import triangulate_ref as R

SETTINGS = [(ncam, use_ransac, mv) for ncam in (12, 5) for use_ransac in (True, False) for mv in (2, 3)]


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def key(ncam, use_ransac, mv):
    return f"all_c{ncam}_{'ransac' if use_ransac else 'dlt'}_mv{mv}"


@pytest.mark.parametrize("ncam,use_ransac,mv", SETTINGS)
def test_restatement_reproduces_the_reference(fx, ncam, use_ransac, mv):
    P, obs, scores = R.fixture_arrays(fx, ncam)
    res = R.solve_all(P, obs, scores, conf=float(fx["confidence_threshold"]), min_views=mv, thr=float(fx["reproj_threshold"]),
                      use_ransac=use_ransac)
    tracks, stats = fx[key(ncam, use_ransac, mv) + "_tracks"][:, 0], dict(zip(fx["stat_keys"], fx[key(ncam, use_ransac, mv) + "_stats"]))
    status = R.field(res, "status")
    assert np.array_equal(status == 0, np.isfinite(tracks).all(axis=-1))
    assert (status == 1).sum() == stats["failed_insufficient_views"] and (status == 2).sum() == stats["failed_ransac"]
    ok = status == 0
    xyz = R.field(res, "xyz")
    rel = np.abs(xyz[ok] - tracks[ok]).max(axis=-1) / np.abs(tracks[ok]).max(axis=-1)
    assert rel.max() <= 1e-9, rel.max()
    used = R.field(res, "views_used")[ok]
    assert used.mean() == pytest.approx(stats["mean_views_used"], rel=1e-12)  # the counts are integers: equal means, equal counts
    errs = R.field(res, "mean_err")[ok]
    assert errs.mean() == pytest.approx(stats["mean_reproj_error_px"], rel=1e-9)
    assert np.median(errs) == pytest.approx(stats["median_reproj_error_px"], rel=1e-9)
    assert R.ambiguous(res, float(fx["reproj_threshold"])) == 0
    if ncam == 12 and use_ransac and mv == 2:  # every status occurs, and the seeded subset of hypotheses is in use
        assert {0, 1, 2} <= set(status.ravel().tolist()) and max(r["n"] for r in res.ravel()) == 12


def test_restatement_reproduces_the_single_problems(fx):
    for i in range(len(fx["single_n"])):
        v = np.flatnonzero(fx["single_views"][i])
        f, k = fx["single_frame_kp"][i]
        Ps, pts = fx["P"][v], fx["coords"][v, f, k]
        mn, n_ref, pt_ref = int(fx["single_min"][i]), int(fx["single_n"][i]), fx["single_pt"][i]
        if len(v) == 2:
            r = R.solve(Ps, pts, min_views=1, use_ransac=False, keep_all=True)
            n = int((r["view_err"] < 15.0).sum())
            got = (r["xyz"], n) if n >= mn else (None, 0)
        else:
            r = R.solve(Ps, pts, min_views=mn, use_ransac=True, keep_all=True)
            got = (r["xyz"], r["views_used"]) if r["status"] == 0 else (None, 0)
            assert R.ambiguous(np.asarray([r], object)) == 0
        assert got[1] == n_ref
        if n_ref:
            assert R.rel_err(got[0], pt_ref) <= 1e-9
        else:
            assert got[0] is None and np.isnan(pt_ref).all()
    sizes = fx["single_views"].sum(axis=1)
    assert 0 in fx["single_n"] and 2 in sizes and sizes.max() >= 11  # a failure, the n = 2 branch, the seeded subset


def test_pair_table(fx):
    from smilify_amd import _lib, triangulate

    table = triangulate.pair_table()
    assert table.shape == (R.MAX_VIEWS + 1, R.MAX_HYP, 2) == (_lib.TRI_MAX_VIEWS + 1, _lib.TRI_MAX_HYP, 2) and table.dtype == np.int32
    all12 = list(itertools.combinations(range(12), 2))
    assert np.array_equal(table[12], np.asarray([all12[i] for i in fx["draw_n12"]]))  # the reference's own draw
    for n in range(2, R.MAX_VIEWS + 1):
        pairs = np.asarray(R.pair_list(n))
        assert len(pairs) == min(n * (n - 1) // 2, 50)
        assert np.array_equal(table[n, :len(pairs)], pairs) and not table[n, len(pairs):].any()
        assert (pairs[:, 0] < pairs[:, 1]).all()
        assert pairs.max() < n and len({tuple(p) for p in pairs}) == len(pairs)
    assert np.array_equal(table[10, :45], np.asarray(list(itertools.combinations(range(10), 2))))  # 45 pairs: all, in order
    assert not np.array_equal(table[11, :50], np.asarray(list(itertools.combinations(range(11), 2)))[:50])  # 55 pairs: the draw


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_generated_gpu_cases_are_unambiguous(name):
    """Cap: 0 problems with a hypothesis whose view lies within 1e-6 px of the threshold, so that no GPU disagreement on an inlier
    can be a borderline one (1 px of noise against > 100 px outliers and a 15 px threshold: the margins are whole pixels)."""
    c = cases.get(name)
    assert R.ambiguous(c["res"], c["thr"]) == 0
    status = R.field(c["res"], "status")
    assert (status == 0).any()
    if name == "ties":
        for r in c["res"].ravel():  # two hypotheses share the largest count and differ in their inliers: the selection rule decides
            top = np.flatnonzero(r["hyp_count"] == r["hyp_count"].max())
            assert len(top) >= 2 and r["winner"] == top[0]
            masks = {tuple((r["hyp_err"][h] < c["thr"]).tolist()) for h in top}
            assert len(masks) >= 2


def test_argument_checks_without_gpu():
    import ctypes

    from smilify_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(R.GOLDEN)), "include", "smilfit.h")).read()
    assert "#define SMIL_TRI_MAX_VIEWS 32" in header and "#define SMIL_TRI_MAX_HYP 50" in header
    err = lambda: lib.smil_last_error()  # noqa: E731
    one = ctypes.c_void_p(256)  # never dereferenced: every call below fails before a launch

    def call(N=1, Kp=1, C=4, min_views=2, mode=1, P=one, obs=one, pairs=one, K=None, dist=None, out=one):
        return lib.smil_triangulate(P, K, dist, obs, None, pairs, N, Kp, C, 0.3, min_views, 15.0, mode, out, out, out, out, None, None,
                                    None, None)

    assert call(N=0) == -1 and b"N=0" in err()
    assert call(Kp=0) == -1 and b"Kp=0" in err()
    assert call(C=0) == -1 and b"C=0" in err()
    assert call(C=_lib.TRI_MAX_VIEWS + 1) == _lib.E_UNSUPPORTED and b"SMIL_TRI_MAX_VIEWS" in err()
    assert call(C=_lib.TRI_MAX_VIEWS, P=None) == -1 and b"null" in err()
    assert call(N=2 ** 40, Kp=8) == -1 and b"grid" in err()
    assert call(min_views=0) == -1 and b"min_views" in err()
    assert call(mode=4) == -1 and b"mode" in err()
    assert call(obs=None) == -1 and b"null" in err()
    assert call(out=None) == -1 and b"null" in err()
    assert call(K=one) == -1 and b"together" in err()
    assert call(pairs=None) == -1 and b"pair table" in err()


def test_python_checks_without_gpu():
    from smilify_amd import triangulate

    with pytest.raises(NotImplementedError, match="max_hypotheses"):
        triangulate.triangulate_point_ransac(np.zeros((3, 3, 4)), np.zeros((3, 2)), max_hypotheses=20)
    assert triangulate.triangulate_point_ransac(np.zeros((1, 3, 4)), np.zeros((1, 2))) == (None, 0)
    pts = np.arange(6.0).reshape(3, 2)
    assert triangulate.undistort_points(pts, np.eye(3), np.zeros(5)) is pts and triangulate.undistort_points(pts, np.eye(3), None) is pts
    cams = {f"c{i:02d}": dict(K=np.eye(3), dist=np.zeros(5), R=np.eye(3), t=np.zeros((3, 1))) for i in range(33)}
    with pytest.raises(ValueError, match="SMIL_TRI_MAX_VIEWS"):
        triangulate.triangulate_all(cams, {n: np.zeros((1, 1, 2)) for n in cams}, {n: np.zeros((1, 1)) for n in cams}, 1, 1, verbose=False)
    # P = K [R | t] and the FoV camera's pixel projection, against their definitions
    rng = np.random.default_rng(0)
    cam = dict(K=np.array([[900.0, 0, 640], [0, 910.0, 512], [0, 0, 1]]), R=np.linalg.qr(rng.normal(size=(3, 3)))[0], t=rng.normal(size=(3, 1)))
    assert np.allclose(triangulate.get_projection_matrix(cam), cam["K"] @ np.hstack([cam["R"], cam["t"]]), rtol=0, atol=0)
    Rm, T, X = np.linalg.qr(rng.normal(size=(3, 3)))[0], np.array([0.1, -0.2, 3.0]), rng.uniform(-0.5, 0.5, 3)
    Pm = triangulate.projection_matrix_from_fov_camera(Rm, T, 50.0, 1.25, (480, 640))
    xv = X @ Rm + T
    t = np.tan(np.radians(50.0) / 2)
    x_ndc, y_ndc = xv[0] / (1.25 * t * xv[2]), xv[1] / (t * xv[2])
    h = Pm @ np.append(X, 1.0)
    assert np.allclose(h[:2] / h[2], [320.0 - 320.0 * x_ndc, 240.0 - 240.0 * y_ndc], rtol=1e-13)
    e = triangulate.reprojection_errors_vectorized(Pm[None], X, np.array([[1.0, 2.0]]))
    assert e[0] == pytest.approx(np.hypot(h[0] / h[2] - 1.0, h[1] / h[2] - 2.0)) == triangulate.reprojection_error(Pm, X, [1.0, 2.0])


def test_undistortion_restatement_inverts_the_forward_model():
    """distort(undistort(p)) = p up to what five rounds of the recurrence reach.  The recurrence contracts by about |3 k1 r^2| per
    round, 0.13 at the corner of this image (r^2 = 0.55) and less everywhere else, so five rounds leave at most 0.25^5 < 1e-3 of the
    first round's error, which is the displacement itself.  The observed maximum is recorded in DESIGN.md section 4.6."""
    K = np.array([[1100.0, 0.0, 640.0], [0.0, 1110.0, 512.0], [0.0, 0.0, 1.0]])
    dist = np.array([-0.08, 0.02, 5e-4, -3e-4, -0.004])
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(0, 1280, 400), rng.uniform(0, 1024, 400)], axis=1)
    und = R.undistort5(pts, K, dist)
    moved = np.abs(und - pts).max()
    resid = np.abs(R.distort(und, K, dist) - pts).max()
    print(f"undistortion: displacement up to {moved:.3f} px, residual of five rounds {resid:.3e} px")
    assert 1.0 < moved < 60.0 and resid < 1e-3 * moved
