"""The public triangulation API (smilify_amd/triangulate.py) on the GPU: triangulate_all against the reference's own run
(tests/golden/triangulate_ref.npz), the single-point functions against its ten recorded problems, the camera limit, and the round trip
through this library's own projection."""
import numpy as np
import pytest
import torch

import triangulate_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("ncam,use_ransac,mv", [(n, u, m) for n in (12, 5) for u in (True, False) for m in (2, 3)])
def test_triangulate_all_reproduces_the_reference(ncam, use_ransac, mv):
    from smilify_amd import triangulate

    fx = R.fixture()
    cams, coords, scores = R.fixture_calibration(fx, ncam)
    tracks, stats = triangulate.triangulate_all(cams, coords, scores, 6, 8, confidence_threshold=0.3, min_views=mv, reproj_threshold=15.0,
                                                undistort=True, use_ransac=use_ransac, verbose=False)
    key = f"all_c{ncam}_{'ransac' if use_ransac else 'dlt'}_mv{mv}"
    ref, ref_stats = fx[key + "_tracks"], dict(zip(fx["stat_keys"], fx[key + "_stats"]))
    assert tracks.shape == ref.shape == (6, 1, 8, 3) and tracks.dtype == np.float64
    assert np.array_equal(np.isnan(tracks), np.isnan(ref))
    ok = ~np.isnan(ref).any(axis=-1)
    assert (np.abs(tracks[ok] - ref[ok]).max(axis=-1) / np.abs(ref[ok]).max(axis=-1)).max() <= 1e-9
    assert set(stats) == set(ref_stats)
    for k in ("n_frames", "n_keypoints", "n_cameras", "total_keypoints", "triangulated", "failed_insufficient_views", "failed_ransac"):
        assert stats[k] == ref_stats[k], k
    for k in ("pct_triangulated", "mean_views_used", "mean_reproj_error_px", "median_reproj_error_px"):
        assert stats[k] == pytest.approx(ref_stats[k], rel=1e-9), k
    # frame_indices: a subset, out of order, one beyond every camera
    sub, _ = triangulate.triangulate_all(cams, coords, scores, 6, 8, min_views=mv, use_ransac=use_ransac, verbose=False,
                                         frame_indices=np.array([4, 1, 7]))
    assert np.array_equal(sub[:2], tracks[[4, 1]], equal_nan=True) and np.isnan(sub[2]).all()


def test_single_point_functions_reproduce_the_reference():
    from smilify_amd import triangulate

    fx = R.fixture()
    for i in range(len(fx["single_n"])):
        v = np.flatnonzero(fx["single_views"][i])
        f, k = fx["single_frame_kp"][i]
        Ps, pts = fx["P"][v], fx["coords"][v, f, k]
        pt, n = triangulate.triangulate_point_ransac(Ps, pts, reproj_threshold=15.0, min_inliers=int(fx["single_min"][i]))
        assert n == int(fx["single_n"][i])
        if n == 0:
            assert pt is None
            continue
        assert R.rel_err(pt, fx["single_pt"][i]) <= 1e-9
    v = np.flatnonzero(fx["single_views"][2])
    f, k = fx["single_frame_kp"][2]
    X = triangulate.triangulate_point_dlt(list(fx["P"][v]), list(fx["coords"][v, f, k]))
    assert R.rel_err(X, R.dlt(fx["P"][v], fx["coords"][v, f, k])) <= 1e-9


def test_more_cameras_than_the_limit():
    from smilify_amd import _lib, triangulate

    C = _lib.TRI_MAX_VIEWS + 1
    with pytest.raises(ValueError, match="SMIL_TRI_MAX_VIEWS"):
        triangulate.triangulate_arrays(np.zeros((C, 3, 4)), np.zeros((1, 1, C, 2)))
    with pytest.raises(ValueError, match="SMIL_TRI_MAX_VIEWS"):
        triangulate.triangulate_point_dlt(np.zeros((C, 3, 4)), np.zeros((C, 2)))


def test_round_trip_through_the_renderer_projection(golden):
    """The reference's check on its projection convention (tests/test_triangulation_consistency.py:254-298) on this library's own
    parts: the STICK joints -> Renderer(joints_only=True) through 4 look-at views -> projection_matrix_from_fov_camera ->
    triangulate_all -> the joints again, within the reference's bounds (0.05 max, 0.01 mean)."""
    from smilify_amd import triangulate
    from smilify_amd.cameras import look_at_view_transform
    from smilify_amd.p3d_renderer import Renderer

    S, V = 512, 4
    joints = torch.from_numpy(golden("lbs_stick")["fixture_joints"]).float().to(DEV)  # (2, 55, 3)
    B, J = joints.shape[0], joints.shape[1]
    az = torch.linspace(0, 360, V + 1)[:V]
    Rm, T = look_at_view_transform(3.0, torch.full_like(az, 15.0), az)
    fov = torch.full((V,), 60.0)
    rend = Renderer(S, DEV, views=V)
    rend.set_camera_parameters(Rm, T, fov)
    _, yx = rend(joints, joints, None, joints_only=True)  # (B V, J, 2), image = frame * views + view
    yx = yx.detach().cpu().numpy().astype(np.float64).reshape(B, V, J, 2)
    cams = {f"view{v}": dict(P=triangulate.projection_matrix_from_fov_camera(Rm[v], T[v], 60.0, 1.0, S)) for v in range(V)}
    coords = {f"view{v}": yx[:, v, :, ::-1].copy() for v in range(V)}  # (x, y)
    scores = {f"view{v}": np.ones((B, J)) for v in range(V)}
    tracks, stats = triangulate.triangulate_all(cams, coords, scores, B, J, reproj_threshold=2.0, verbose=False)
    assert stats["triangulated"] == B * J and stats["mean_views_used"] == V
    err = np.linalg.norm(tracks[:, 0] - joints.cpu().numpy(), axis=-1)
    print(f"round trip: max {err.max():.3e} mean {err.mean():.3e}, mean reprojection error {stats['mean_reproj_error_px']:.3e} px")
    assert err.max() < 0.05 and err.mean() < 0.01, (err.max(), err.mean())
