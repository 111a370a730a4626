"""Principal points and crop windows, the parts that need no GPU: the host-side conversions in float64, the table checks of
``engine.CameraSet.struct`` and the argument check of the C ABI (which runs before any launch)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pinhole_ref


def _calibration(S, seed, cx=None, cy=None):
    """One pinhole camera whose R and t are float32 numbers (``opencv_to_fov_camera`` hands R and T out as float32: a calibration
    that float32 holds exactly converts without rounding, and the float64 comparison below then sees the conversion alone)."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    R_cv = (Ry @ Rx).astype(np.float32).astype(np.float64)
    t_cv = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(2.5, 4.0)]).astype(np.float32).astype(np.float64)
    fx, fy = rng.uniform(1.2, 2.0) * S, rng.uniform(1.2, 2.0) * S
    K = np.array([[fx, 0, rng.uniform(0.2, 0.8) * S if cx is None else cx], [0, fy, rng.uniform(0.2, 0.8) * S if cy is None else cy], [0, 0, 1.0]])
    return R_cv, t_cv, K


@pytest.mark.parametrize("window", [None, (301.25, -40.5, 80.0)])
def test_pinhole_camera_reproduces_k_r_t_in_float64(window):
    """opencv_to_pinhole_camera -> projection_matrix_from_fov_camera(principal_point=) is K [R | t] (of the crop window's K when
    there is one) up to scale, to 1e-12 of the matrix's largest entry."""
    from smilify_amd import cameras, triangulate

    S = 512
    for seed in range(4):
        R_cv, t_cv, K = _calibration(1280 if window else S, seed)
        R, T, fov, aspect, pp = cameras.opencv_to_pinhole_camera(R_cv, t_cv, K, S, window=window)
        assert pp.dtype == np.float64 and pp.shape == (2,)
        P = triangulate.projection_matrix_from_fov_camera(R, T, fov, aspect, S, principal_point=pp)
        Kw = K if window is None else cameras.crop_intrinsics(K, window, S)
        want = Kw @ np.hstack([R_cv, t_cv[:, None]])
        P, want = P / np.linalg.norm(P[2, :3]), want / np.linalg.norm(want[2, :3])
        assert np.abs(P - want).max() <= 1e-12 * np.abs(want).max(), np.abs(P - want).max() / np.abs(want).max()
    # without the keyword the matrix is what it was: the centred camera
    Pc = triangulate.projection_matrix_from_fov_camera(R, T, fov, aspect, S)
    assert np.array_equal(Pc, triangulate.projection_matrix_from_fov_camera(R, T, fov, aspect, S, principal_point=None))
    assert np.array_equal(Pc, triangulate.projection_matrix_from_fov_camera(R, T, fov, aspect, S, principal_point=(0.0, 0.0)))


def test_centred_calibration_gives_zero_principal_point_and_the_fov_camera():
    from smilify_amd import cameras

    for S in (64, 512, 513):
        R_cv, t_cv, K = _calibration(S, 7, cx=S / 2, cy=S / 2)
        R, T, fov, aspect, pp = cameras.opencv_to_pinhole_camera(R_cv, t_cv, K, S)
        assert pp[0] == 0.0 and pp[1] == 0.0
        R0, T0, fov0, aspect0 = cameras.opencv_to_fov_camera(R_cv, t_cv, K, (S, S))
        assert R.dtype == R0.dtype and T.dtype == T0.dtype and np.array_equal(R, R0) and np.array_equal(T, T0)
        assert fov == fov0 and aspect == aspect0  # (python floats: bit for bit)


def test_crop_window_maps_pinhole_pixels_to_pinhole_pixels():
    """crop_points_yx of the whole-image projection = the projection through crop_intrinsics, for fractional windows and windows
    that reach past the image (float64: 1e-9 px on coordinates of ~1e3 px is 1e4 roundings)."""
    from smilify_amd import cameras

    rng = np.random.default_rng(3)
    R_cv, t_cv, K = _calibration(1280, 11)
    X = rng.uniform(-0.5, 0.5, (50, 3))
    u, v = pinhole_ref.pinhole_pixels(X, R_cv, t_cv, K)
    for window, S in (((301.25, 140.5, 80.0), 128), ((-33.3, 900.7, 411.1), 64), ((0.0, 0.0, 1280.0), 1280)):
        Kw = cameras.crop_intrinsics(K, window, S)
        s = S / window[2]
        assert Kw[0, 0] == s * K[0, 0] and Kw[1, 1] == s * K[1, 1] and Kw[0, 2] == s * (K[0, 2] - window[0]) and Kw[1, 2] == s * (K[1, 2] - window[1])
        assert np.array_equal(Kw[2], K[2]) and Kw[0, 1] == 0.0 and K is not Kw
        uw, vw = pinhole_ref.pinhole_pixels(X, R_cv, t_cv, Kw)
        yx = cameras.crop_points_yx(np.stack([v, u], -1), window, S)
        np.testing.assert_allclose(yx, np.stack([vw, uw], -1), rtol=0, atol=1e-9)
        yx_t = cameras.crop_points_yx(torch.from_numpy(np.stack([v, u], -1)), window, S)
        assert isinstance(yx_t, torch.Tensor) and yx_t.dtype == torch.float64
        np.testing.assert_allclose(yx_t.numpy(), yx, rtol=0, atol=1e-12)
    assert np.array_equal(cameras.crop_intrinsics(K, (0.0, 0.0, 1280.0), 1280), K)  # the whole image is no crop


def test_camera_set_checks_the_principal_table():
    from smilify_amd import _lib, engine

    views, N, S = 3, 6, 64
    R, T, fov = torch.eye(3)[None].repeat(views, 1, 1), torch.zeros(views, 3), torch.full((views,), 60.0)
    assert engine.CameraSet(R, T, fov, None, views, S).principal is None  # the last field, optional: positional callers stay valid
    c = engine.CameraSet(R, T, fov, None, views, S).struct(N)
    assert not c.principal and c.nPrincipal == 0
    for k in (1, views, N):
        pp = torch.zeros(k, 2)
        c = engine.CameraSet(R, T, fov, None, views, S, pp).struct(N)
        assert c.principal == pp.data_ptr() and c.nPrincipal == k
    with pytest.raises(_lib.SmilError, match="principal"):
        engine.CameraSet(R, T, fov, None, views, S, torch.zeros(2, 2)).struct(N)
    with pytest.raises(_lib.SmilError, match="principal"):
        engine.CameraSet(R, T, fov, None, views, S, torch.zeros(views, 3)).struct(N)
    with pytest.raises(_lib.SmilError, match="principal"):
        engine.CameraSet(R, T, fov, None, views, S, torch.zeros(views, 2, dtype=torch.float64)).struct(N)
    with pytest.raises(NotImplementedError, match="gradient"):
        engine.CameraSet(R, T, fov, None, views, S, torch.zeros(views, 2, requires_grad=True)).struct(N)
    assert ctypes.sizeof(_lib.Cameras) == 96  # three int32 + pad, then five (pointer, int32 + pad) pairs


def test_c_abi_rejects_an_empty_principal_table_before_any_launch():
    from smilify_amd import _lib

    lib = _lib.load()
    assert b"0.4" in lib.smil_version()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smilfit.h")).read()
    assert "const float *principal;" in header and "int32_t nPrincipal;" in header
    assert header.index("int32_t nAspect;") < header.index("const float *principal;") < header.index("} SmilCameras;")
    one = ctypes.c_void_p(256)  # never dereferenced: every call below fails before a launch
    c = _lib.Cameras()
    c.N, c.views, c.S = 2, 1, 32
    c.R, c.nR, c.T, c.nT, c.fov, c.nFov = one, 1, one, 1, one, 1
    c.principal, c.nPrincipal = one, 0
    assert lib.smil_project(ctypes.byref(c), one, 4, one, one, None) == -1
    assert b"principal" in lib.smil_last_error() and b"smil_project" in lib.smil_last_error()
    c.nPrincipal = -3
    assert lib.smil_project_backward(ctypes.byref(c), one, 4, one, one, one, one, 0, None, None) == -1
    assert b"principal" in lib.smil_last_error() and b"nPrincipal=-3" in lib.smil_last_error()


def test_renderer_rejects_a_principal_point_that_wants_a_gradient():
    """(The check sits in front of the GPU: ``_principal_table`` is plain host code.)"""
    from smilify_amd.p3d_renderer import Renderer

    r = Renderer.__new__(Renderer)
    r.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="gradient"):
        r._principal_table(torch.zeros(3, 2, requires_grad=True))
    with pytest.raises(ValueError, match="principal_point"):
        r._principal_table(torch.zeros(3, 3))
    assert r._principal_table(None) is None
    pp = r._principal_table([0.25, -0.5])
    assert pp.shape == (1, 2) and pp.dtype == torch.float32 and pp.is_contiguous()
