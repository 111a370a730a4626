"""Principal points and crop windows on the HIP path (``pytest -m gpu``): ``smil_project`` and its backward, the fused per-frame
forward and backward, the Renderer (silhouette, joints, colour), a crop window, the fitter (one evaluation, the captured graph, the
epoch cache) and the round trip through ``triangulate_all``.  References: the OpenCV pinhole model in float64 and
``tests/pinhole_ref.py``.  Every bound is the one an existing test uses for the same quantity (named at its use)."""
import numpy as np
import pytest
import torch

import colour_cases
import pinhole_ref
import shade_ref
import test_gpu_cameras as tc
from conftest import oracle_model
from oracle import fitter_ref, render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans", "fov")


def _off_centre(cal, S, pp):
    """The calibrations with the principal points that the NDC offsets ``pp`` (n,2) stand for: cx = (S/2)(1 - px)."""
    out = []
    for (R, t, K), (px, py) in zip(cal, np.asarray(pp, np.float64)):
        K = K.copy()
        K[0, 2], K[1, 2] = 0.5 * S * (1.0 - px), 0.5 * S * (1.0 - py)
        out.append((R, t, K))
    return out


@pytest.mark.parametrize("k", ["one", "views", "images"])
def test_projection_with_a_principal_table(k):
    """engine.project / project_backward / fov_reduce with tables of 1, views and N rows (257 points: one past a 256-thread block;
    aspect != 1; offsets up to 0.6 NDC and one outside [-1, 1]) against the float64 pinhole model (2e-2 px) and pinhole_ref (2e-3 px
    forward; rtol 2e-4, atol 2e-3 on d_pts; rtol 2e-4, atol 1e-3 on d_fov): the bounds of test_hip_projection_reproduces_pinhole_with_aspect.
    d_fov and the depth part of d_pts are where a backward that read the stored, shifted NDC would show."""
    from smilify_amd import engine

    S, frames, views, P = 512, 2, 3, 257
    N = frames * views
    cal = tc._calibrations(views, S, seed=2)
    R, T, fov, aspect = tc._fov_cameras(cal, S)
    assert float((aspect - 1).abs().min()) > 1e-3
    rng = np.random.default_rng(5)
    pp = rng.uniform(-0.6, 0.6, ({"one": 1, "views": views, "images": N}[k], 2))
    pp[-1, 0] = 1.3  # a principal point outside the image (a crop window beside the optical axis)
    pp = torch.tensor(pp, dtype=torch.float32)
    X = rng.uniform(-0.5, 0.5, (frames, P, 3)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    cams = engine.CameraSet(R.to(DEV).contiguous(), T.to(DEV).contiguous(), fov.to(DEV), aspect.to(DEV), views, S, pp.to(DEV))
    ndc, yx = engine.project(cams, Xd)
    yx_h = yx.cpu().numpy()
    ppN = pinhole_ref.rows(pp, N).numpy()
    for n in range(N):
        R_cv, t_cv, K = _off_centre([cal[n % views]], S, ppN[n:n + 1])[0]
        u, v = pinhole_ref.pinhole_pixels(X[n // views], R_cv, t_cv, K)
        np.testing.assert_allclose(yx_h[n, :, 0], v, atol=2e-2)
        np.testing.assert_allclose(yx_h[n, :, 1], u, atol=2e-2)
    Xo = torch.from_numpy(X).double().requires_grad_()
    fov_o = fov.double().requires_grad_()
    rw = lambda t: pinhole_ref.rows(t, N)  # noqa: E731
    ndc_o = pinhole_ref.project_to_ndc(Xo[torch.arange(N) // views], rw(R), rw(T), rw(fov_o), rw(aspect), rw(pp))
    yx_o = pinhole_ref.ndc_to_screen(ndc_o, S)
    np.testing.assert_allclose(yx_h, yx_o.detach().numpy(), atol=2e-3)
    np.testing.assert_allclose(ndc.cpu().numpy()[..., :2], ndc_o.detach().numpy()[..., :2], atol=2e-3 / (S / 2))  # (the same bound, in NDC)
    np.testing.assert_allclose(ndc.cpu().numpy()[..., 2], ndc_o.detach().numpy()[..., 2], atol=1e-5)
    w_yx = torch.from_numpy(rng.standard_normal((N, P, 2)).astype(np.float32))
    w_ndc = torch.from_numpy(rng.standard_normal((N, P, 2)).astype(np.float32))
    ((yx_o * w_yx.double()).sum() + (ndc_o[..., :2] * w_ndc.double()).sum()).backward()
    d_pts, d_fov_img = engine.project_backward(cams, Xd, d_ndc=w_ndc.to(DEV).contiguous(), d_yx=w_yx.to(DEV).contiguous())
    d_fov = engine.fov_reduce(cams, d_fov_img)
    print(f"max |d_pts - ref| {np.abs(d_pts.cpu().numpy() - Xo.grad.numpy()).max():.3e} of {Xo.grad.abs().max():.3e}; "
          f"d_fov {d_fov.cpu().numpy()} ref {fov_o.grad.numpy()}")
    np.testing.assert_allclose(d_pts.cpu().numpy(), Xo.grad.numpy(), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(d_fov.cpu().numpy(), fov_o.grad.numpy(), rtol=2e-4, atol=1e-3)
    # the backward does not read the table at all: the same bits without it
    plain = engine.CameraSet(cams.R, cams.T, cams.fov, cams.aspect, views, S)
    d_pts0, d_fov_img0 = engine.project_backward(plain, Xd, d_ndc=w_ndc.to(DEV).contiguous(), d_yx=w_yx.to(DEV).contiguous())
    assert torch.equal(d_pts, d_pts0)
    # (an image's sum is two blocks' partial sums added by float atomics in their order of arrival: one rounding of a sum of ~1e3)
    np.testing.assert_allclose(d_fov_img.cpu().numpy(), d_fov_img0.cpu().numpy(), rtol=0, atol=1e-6 * float(d_fov_img0.abs().max()))
    # a table of zeros is the centred camera plus an exact zero
    zero = engine.CameraSet(cams.R, cams.T, cams.fov, cams.aspect, views, S, torch.zeros_like(cams.principal))
    ndc_z, yx_z = engine.project(zero, Xd)
    ndc_c, yx_c = engine.project(plain, Xd)
    assert torch.equal(ndc_z, ndc_c) and torch.equal(yx_z, yx_c)


def _lbs_case(tables, key, views, B, S=96):
    from smilify_amd import cameras as cam_mod
    from smilify_amd import engine as eng

    dm = eng.DeviceModel(tables(key), DEV)
    g = torch.Generator().manual_seed(8)
    beta = (0.4 * torch.randn(dm.nB, generator=g)).to(DEV)
    theta = (0.25 * torch.randn(B, dm.J, 3, generator=g)).to(DEV)
    trans = (0.1 * torch.randn(B, 3, generator=g)).to(DEV)
    pp = (0.5 * torch.rand(views, 2, generator=g) - 0.25).to(DEV)
    R, T = cam_mod.look_at_view_transform(3.0, 10.0, np.linspace(0, 300, views), device=DEV)
    cams = eng.CameraSet(R.contiguous(), T.contiguous(), torch.full((views,), 50.0, device=DEV), None, views, S, pp)
    return eng, dm, beta, theta, trans, cams


@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("key", ["stick", "synthetic", "synthetic_static", "mouse"])
def test_fused_forward_with_a_principal_table_equals_forward_then_projection(key, views, tables):
    """smil_lbs_forward_project with a principal table = smil_lbs_forward followed by smil_project, torch.equal on every output, for
    the model keys of test_forward_with_projection_equals_forward_then_projection and views in {1, 3}.  (The fused per-frame kernel
    agrees with the separate kernels to the last bit but one only - verts 1.2e-7, ndc 4.8e-7, yx 1.1e-5 px measured - so with a table
    the entry point runs the separate kernels; the centred call keeps the fused kernel and its older test's 1e-6.)"""
    B = 5
    eng, dm, beta, theta, trans, cams = _lbs_case(tables, key, views, B)
    kw = dict(trans=trans, shared_beta=True, trans_after_joints=True)
    ref = eng.lbs_forward(dm, beta, theta, **kw)
    ref["ndc"], ref["yx"] = eng.project_verts_and_joints(cams, ref["verts"], ref["joints"])
    got = eng.lbs_forward(dm, beta, theta, project=dict(cams=cams, ndc=True, yx=True), **kw)
    names = ("v_shaped", "J_rest", "Rs", "G", "A", "new_J", "verts", "joints", "ndc", "yx")
    for n in names:
        print(f"{key} views={views} {n}: max |with projection - separate| {(got[n] - ref[n]).abs().max().item():.3e} of {ref[n].abs().max().item():.3e}")
    for n in names:
        assert torch.equal(got[n], ref[n]), n
    # one output at a time: the single-set launches of smil_project give the same bits as the two-set launch
    only_ndc = eng.lbs_forward(dm, beta, theta, project=dict(cams=cams, ndc=True, yx=False), **kw)
    only_yx = eng.lbs_forward(dm, beta, theta, project=dict(cams=cams, ndc=False, yx=True), **kw)
    assert "yx" not in only_ndc and "ndc" not in only_yx
    assert torch.equal(only_ndc["ndc"], ref["ndc"]) and torch.equal(only_yx["yx"], ref["yx"])
    # the offset is added behind the division, where nothing contracts with it: the centred coordinates plus one rounding
    plain = eng.CameraSet(cams.R, cams.T, cams.fov, None, views, cams.S)
    ndc_c, yx_c = eng.project_verts_and_joints(plain, ref["verts"], ref["joints"])
    ppN = cams.principal[torch.arange(B * views, device=DEV) % views]
    assert torch.equal(got["ndc"][..., :2], ndc_c[..., :2] + ppN[:, None, :]) and torch.equal(got["ndc"][..., 2], ndc_c[..., 2])
    assert float((got["yx"] - yx_c).abs().max()) > 1.0  # (the offsets are pixels, not roundings)


def test_a_table_of_zeros_gives_the_separate_kernels_bits(tables):
    """The centred call takes the fused per-frame kernel (B = 5: its 1024-thread form; B = 300, more frames than CUs: the 512-thread
    one) and stays within the 1e-6 of test_forward_with_projection_equals_forward_then_projection; the same call with a table of zeros
    takes the separate kernels and gives the bits of the centred separate route (x + 0 is x)."""
    for B in (5, 300):
        eng, dm, beta, theta, trans, cams = _lbs_case(tables, "synthetic", 3, B)
        kw = dict(trans=trans, shared_beta=True, trans_after_joints=True)
        plain = eng.CameraSet(cams.R, cams.T, cams.fov, None, 3, cams.S)
        zero = eng.CameraSet(cams.R, cams.T, cams.fov, None, 3, cams.S, torch.zeros_like(cams.principal))
        ref = eng.lbs_forward(dm, beta, theta, **kw)
        ref["ndc"], ref["yx"] = eng.project_verts_and_joints(plain, ref["verts"], ref["joints"])
        fused = eng.lbs_forward(dm, beta, theta, project=dict(cams=plain, ndc=True, yx=True), **kw)
        tabled = eng.lbs_forward(dm, beta, theta, project=dict(cams=zero, ndc=True, yx=True), **kw)
        for n in ("verts", "joints", "ndc", "yx"):
            err = (fused[n] - ref[n]).abs().max().item() / ref[n].abs().max().item()
            assert err <= 1e-6, (n, err)
            assert torch.equal(tabled[n], ref[n]), n


@pytest.mark.parametrize("key,views", [("stick", 1), ("synthetic", 3)])
def test_fused_backward_does_not_read_the_principal_table(key, views, tables):
    """smil_lbs_backward_ndc: bit-equal gradients with and without a principal table, from the same saved outputs and the same
    upstream d_ndc / d_yx.  (The per-image fov sums are the one output that two calls on identical cameras do not repeat bit for
    bit either: the waves of a frame add their partial sums with float atomics in their order of arrival.  Up to sixteen
    roundings of a partial sum: 1e-6 of the largest sum.)"""
    eng, dm, beta, theta, trans, cams = _lbs_case(tables, key, views, 5)
    assert eng.lbs_backward_ndc_supported(dm, dm.nB, views)
    saved = eng.lbs_forward(dm, beta, theta, trans=trans, shared_beta=True, trans_after_joints=True)
    N = 5 * views
    g = torch.Generator().manual_seed(3)
    d_ndc = torch.randn(N, dm.V, 2, generator=g).to(DEV)
    d_yx = torch.randn(N, dm.J, 2, generator=g).to(DEV)
    plain = eng.CameraSet(cams.R, cams.T, cams.fov, None, views, cams.S)
    out = []
    for c in (cams, plain):
        fov_img = torch.zeros(N, device=DEV)
        r = eng.lbs_backward(dm, saved, None, None, ndc_upstream=dict(cams=c, d_ndc=d_ndc, d_ndc_scale=None, d_yx=d_yx, d_fov_img=fov_img))
        out.append({**{n: t for n, t in r.items() if isinstance(t, torch.Tensor)}, "d_fov_img": fov_img})
    assert set(out[0]) == set(out[1]) and {"d_beta", "d_theta", "d_trans", "d_joints", "d_fov_img"} <= set(out[0])
    for n in out[0]:
        assert float(out[0][n].abs().max()) > 0, n
        if n == "d_fov_img":
            np.testing.assert_allclose(out[0][n].cpu().numpy(), out[1][n].cpu().numpy(), rtol=0, atol=1e-6 * float(out[1][n].abs().max()))
        else:
            assert torch.equal(out[0][n], out[1][n]), n


def _posed_mesh(t, n, seed=2):
    from smilify_amd.smal_torch import SMAL

    smal = SMAL(DEV, tables=t)
    theta = 0.2 * torch.randn(n, t.J, 3, generator=torch.Generator().manual_seed(seed))
    verts, joints, _, _ = smal(torch.zeros(n, t.nB, device=DEV), theta.to(DEV))
    return smal, verts.detach(), joints.detach()


def test_renderer_with_a_principal_point(tables):
    """Renderer.set_camera_parameters(..., principal_point=) at S = 64, n = 3: joints like the pinhole model (5e-3 px), the
    silhouette against pinhole_ref (mean < 5e-6, max < 2e-3: the bounds of test_renderer_aspect_branch), joints_only the same bits."""
    from smilify_amd.p3d_renderer import Renderer

    t = tables("synthetic")
    S, n = 64, 3
    pp = torch.tensor([[0.3, -0.2], [-0.45, 0.1], [0.05, 0.5]])
    cal = tc._calibrations(n, S, seed=4)
    R, T, fov, aspect = tc._fov_cameras(cal, S)
    smal, verts, joints = _posed_mesh(t, n)
    rend = Renderer(S, DEV)
    rend.set_camera_parameters(R, T, fov, aspect_ratio=aspect, principal_point=pp)
    assert rend.cameras.principal_point.shape == (n, 2) and rend.cameras.principal_point.device.type == "cuda"
    sil, proj = rend(verts, joints, smal.faces)
    _, proj_only = rend(verts, joints, smal.faces, joints_only=True)
    assert torch.equal(proj, proj_only)
    J = joints.cpu().numpy().astype(np.float64)
    for i, (R_cv, t_cv, K) in enumerate(_off_centre(cal, S, pp.numpy())):
        u, v = pinhole_ref.pinhole_pixels(J[i], R_cv, t_cv, K)
        np.testing.assert_allclose(proj[i, :, 0].cpu().numpy(), v, atol=5e-3)
        np.testing.assert_allclose(proj[i, :, 1].cpu().numpy(), u, atol=5e-3)
    sil_o, proj_o = pinhole_ref.PinholeRenderer(S, R, T, fov, aspect, pp)(verts.cpu(), joints.cpu(), smal.faces.cpu())
    np.testing.assert_allclose(proj.cpu().numpy(), proj_o.numpy(), atol=5e-3)
    d = (sil.cpu() - sil_o).abs().numpy()
    cen, _ = render_ref.OracleRenderer(S, R, T, fov, aspect)(verts.cpu(), joints.cpu(), smal.faces.cpu())
    print(f"sil: sum {float(sil_o.sum()):.1f} mean |d| {d.mean():.3e} max |d| {d.max():.3e}; mean |shifted - centred| {float((sil_o - cen).abs().mean()):.3e}")
    assert sil_o.sum() > 10 and d.mean() < 5e-6 and d.max() < 2e-3, (float(sil_o.sum()), d.mean(), d.max())
    assert float((sil_o - cen).abs().mean()) > 1e-3  # (the offsets do move the silhouette: the comparison above is of shifted images)
    with pytest.raises(ValueError, match="principal_point"):  # a table of 2 rows for 3 images
        rend.set_camera_parameters(R, T, fov, aspect_ratio=aspect, principal_point=pp[:2])
        rend(verts, joints, smal.faces, joints_only=True)
    with pytest.raises(NotImplementedError, match="gradient"):
        rend.set_camera_parameters(R, T, fov, principal_point=pp.clone().requires_grad_())


def test_colour_image_with_a_per_image_principal_table(tables):
    """render_colour with views = 2 and one table row per image, cut into launches of one frame so that the per-launch slicing of
    the camera tables is taken, against tests/shade_ref.py fed the shifted NDC: at most 1e-3 of the pixels off, the bound of
    test_gpu_colour.py."""
    import test_gpu_colour as tcol
    from smilify_amd import engine

    t = tables("synthetic")
    S, frames, views = 64, 3, 2
    N = frames * views
    verts = tcol._posed(t, frames, seed=9).to(DEV)
    cams = tcol._cams(views, frames, S, aspect=1.3)
    g = torch.Generator().manual_seed(4)
    cams.principal = (0.8 * torch.rand(N, 2, generator=g) - 0.4).to(DEV)
    dm = engine.DeviceModel(t, DEV)
    ndc, _ = engine.project(cams, verts, want_yx=False)
    plain, _ = engine.project(engine.CameraSet(cams.R, cams.T, cams.fov, cams.aspect, views, S), verts, want_yx=False)
    assert torch.equal(ndc[..., :2], plain[..., :2] + cams.principal[:, None, :])
    whole, p2f_whole = engine.render_colour(dm, cams, verts, tcol.RGB, verts_ndc=ndc, want_pix_to_face=True)
    limit = engine.MAX_COLOUR_WORKSPACE_BYTES
    try:  # one frame per launch: rows() slices the per-image tables, the principal table among them
        engine.MAX_COLOUR_WORKSPACE_BYTES = int(engine._lib.load().smil_colour_workspace_bytes(dm.handle, views, S))
        img, p2f = engine.render_colour(dm, cams, verts, tcol.RGB, want_pix_to_face=True)  # (projects by itself, launch by launch tables)
    finally:
        engine.MAX_COLOUR_WORKSPACE_BYTES = limit
    torch.cuda.synchronize()
    assert torch.equal(img, whole) and torch.equal(p2f, p2f_whole)
    ndc_h, img_h, p2f_h, vw = ndc.double().cpu().numpy(), img.cpu().numpy(), p2f.cpu().numpy(), verts.cpu().numpy()
    Rh, Th = cams.R.cpu().numpy(), cams.T.cpu().numpy()
    bad = hits = 0
    for n in range(N):
        ref, rp, unsure = shade_ref.render_colour(vw[n // views], ndc_h[n], t.faces, Rh[n % Rh.shape[0]], Th[n % Th.shape[0]], tcol.RGB, S)
        b, h, _, _ = colour_cases.compare_image(img_h[n], p2f_h[n], ref, rp, unsure, t.F)
        bad, hits = bad + b, hits + h
    print(f"colour: {bad} pixels off, {hits} compared hits")
    assert bad <= 1e-3 * N * S * S and hits > 100, (bad, hits)


def test_crop_window_camera(tables):
    """Joints through the window camera = crop_points_yx of the joints through the whole-image camera, 1e-2 px (the multi-view
    bound of test_batched_multiview_joint_projection).  S = 128, a window of side 80 at a non-integer origin of a 1280-px frame."""
    from smilify_amd import cameras
    from smilify_amd.p3d_renderer import Renderer

    t = tables("synthetic")
    S, B, V, src, side = 128, 3, 4, 1280, 80.0
    cal = [(R, tt, np.array([[K[0, 0] * src / S, 0, 0.47 * src], [0, K[1, 1] * src / S, 0.52 * src], [0, 0, 1.0]])) for R, tt, K in tc._calibrations(V, S, seed=9)]
    off_axis = torch.tensor([0.45, 0.25, 0.0])  # the animal stands beside the optical axes: its window does not hold the principal point
    joints = (0.03 * torch.randn(B, t.J, 3, generator=torch.Generator().manual_seed(5)) + off_axis).to(DEV)  # (~20 px across at this range)

    def project(size, windows):
        conv = [cameras.opencv_to_pinhole_camera(R, tt, K, size, window=w) for (R, tt, K), w in zip(cal, windows)]
        rend = Renderer(size, DEV, views=V)
        rend.set_camera_parameters(torch.tensor(np.stack([c[0] for c in conv])), torch.tensor(np.stack([c[1] for c in conv])),
                                   torch.tensor([c[2] for c in conv], dtype=torch.float32), aspect_ratio=torch.tensor([c[3] for c in conv], dtype=torch.float32),
                                   principal_point=torch.tensor(np.stack([c[4] for c in conv]), dtype=torch.float32))
        yx = rend(joints, joints, None, joints_only=True)[1].cpu().numpy().astype(np.float64)
        return yx.reshape(B, V, t.J, 2), np.stack([c[4] for c in conv])

    whole, _ = project(src, [None] * V)
    centre = whole.mean(axis=(0, 2))  # (V, 2) in (y, x): every camera's window sits on its view of the animal, at a fractional origin
    windows = [(float(c[1]) - 0.5 * side + 0.3, float(c[0]) - 0.5 * side - 0.25, side) for c in centre]
    crop, pp = project(S, windows)
    assert np.abs(pp).max() > 1.0, pp  # (an offset outside [-1, 1])
    Jn = joints.cpu().numpy().astype(np.float64)
    for v, (R_cv, t_cv, K) in enumerate(cal):
        want = cameras.crop_points_yx(whole[:, v], windows[v], S)
        Kw = cameras.crop_intrinsics(K, windows[v], S)
        for b in range(B):
            u, vv = pinhole_ref.pinhole_pixels(Jn[b], R_cv, t_cv, Kw)
            np.testing.assert_allclose(crop[b, v], np.stack([vv, u], -1), atol=1e-2)
        print(f"crop view {v}: principal point {pp[v]}, max |window camera - cropped whole image| {np.abs(crop[:, v] - want).max():.3e} px")
        # (the whole-image side of this comparison is fp32 pixels of a 1280-px image scaled by S / side = 1.6)
        np.testing.assert_allclose(crop[:, v], want, atol=1e-2)
    inside = ((crop > 0) & (crop < S)).all(-1)
    print(f"crop: {int(inside.sum())} of {inside.size} joints inside their windows")
    assert inside.sum() > inside.size // 2


# ---- fitter ------------------------------------------------------------------------------------------------------------------
FIT_PP = torch.tensor([[0.25, -0.15], [-0.3, 0.2], [0.1, 0.35]])


def _fit_problem(t, window, pp=FIT_PP):
    """frames = 2, views = 3, S = 64; cameras with off-centre principal points; targets from pinhole_ref: the hard silhouette and
    the joints of the problem's own parameters with the pose turned a little, through the same cameras."""
    from smilify_amd import synthetic

    frames, views, S = 2, 3, 64
    f = synthetic.make_problem(t, frames, views, S, DEV, radius=2.4, seed=5, window=window)
    f.set_cameras(f.renderer.cameras.R, f.renderer.cameras.T, principal_point=pp)
    case = _fit_problem.targets.get(id(t))
    if case is None:
        m, params, targets, cams = _oracle(f, t)
        tgt = {k: v.clone() for k, v in params.items()}
        g = torch.Generator().manual_seed(77)
        tgt["joint_rotations"] = tgt["joint_rotations"] + 0.08 * torch.randn(tgt["joint_rotations"].shape, generator=g)
        tgt["trans"] = tgt["trans"] + 0.03 * torch.randn(tgt["trans"].shape, generator=g)
        sil = torch.zeros(frames * views, 1, S, S, dtype=torch.uint8)
        tj = torch.zeros(frames * views, t.J, 2)
        with torch.no_grad():
            for v in range(views):
                rend = pinhole_ref.PinholeRenderer(S, cams["R"][v:v + 1], cams["T"][v:v + 1], tgt["fov"], None, FIT_PP[v:v + 1])
                _, _, ex = fitter_ref.fit_losses(m, tgt, range(frames), [1.0] * 6, targets, cams, S, f.mean_betas.cpu(), f.betas_prec.cpu(), renderer=rend)
                sil[v::views] = (ex["sil"] > 0.5).to(torch.uint8)
                tj[v::views] = ex["proj"].float()
        case = _fit_problem.targets[id(t)] = (sil, tj)
    f.sil_imgs, f.target_joints = case[0].to(DEV), case[1].to(DEV)
    return f


_fit_problem.targets = {}


def _oracle(f, t):
    cpu = lambda x: x.detach().cpu().clone()  # noqa: E731
    params = {k: cpu(getattr(f, k)) for k in ("betas", "log_beta_scales", "betas_trans", "global_rotation", "trans", "joint_rotations", "fov")}
    targets = dict(sil=cpu(f.sil_imgs), joints=cpu(f.target_joints), visibility=cpu(f.target_visibility))
    return oracle_model(t), params, targets, dict(R=cpu(f.renderer.cameras.R), T=cpu(f.renderer.cameras.T))


def test_fitter_evaluation_with_principal_points(tables):
    """One evaluation of SMALFitter (frames = 2, views = 3, S = 64) against the oracle's loss block fed by pinhole_ref: the six
    terms within 1e-4 relative (the project's parity bound), the gradients within 5e-3 (max) and 5e-4 (rms) of the largest
    reference entry (the bound of test_fitter_forward_matches_reference_golden)."""
    from smilify_amd import synthetic

    t = tables("synthetic")
    frames, views, S, W = 2, 3, 64, 2
    f = _fit_problem(t, W)
    weights, w_temp = synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL
    objs, grads = f._loss_and_grads(None, weights, w_temp, window=W)
    m, params, targets, cams = _oracle(f, t)
    for k in PARAMS:
        params[k].requires_grad_()
    terms = {k: 0.0 for k in fitter_ref.OBJ_KEYS}
    for v in range(views):
        sel = [fr * views + v for fr in range(frames)]
        tv = {k: x[sel] for k, x in targets.items()}
        rend = pinhole_ref.PinholeRenderer(S, cams["R"][v:v + 1], cams["T"][v:v + 1], params["fov"], None, FIT_PP[v:v + 1])
        _, o, _ = fitter_ref.fit_losses(m, params, range(frames), weights, tv, cams, S, f.mean_betas.cpu(), f.betas_prec.cpu(), renderer=rend)
        for k in terms:
            terms[k] = terms[k] + o[k] / views
    total = sum(terms.values()) + sum(fitter_ref.temporal(params, w_temp))
    total.backward()
    got = objs.cpu().numpy()
    for i, k in enumerate(fitter_ref.OBJ_KEYS):
        print(f"{k}: {got[i]:.7g} reference {float(terms[k].detach()):.7g}")
    for i, k in enumerate(fitter_ref.OBJ_KEYS):
        assert abs(got[i] - float(terms[k].detach())) <= 1e-4 * abs(float(terms[k].detach())), (k, got[i], float(terms[k].detach()))
    assert abs(float(got[:9].sum()) - float(total.detach())) <= 1e-4 * abs(float(total.detach()))
    assert float(terms["sil_reproj"]) > 0 and float(terms["joint"]) > 0
    ref = dict(betas=params["betas"].grad, pose=torch.cat([params["global_rotation"].grad[:, None], params["joint_rotations"].grad], 1),
               trans=params["trans"].grad, log_beta_scales=params["log_beta_scales"].grad, fov=params["fov"].grad)
    for n, r in ref.items():
        r = r.numpy()
        err = np.abs(grads[n].cpu().numpy().reshape(r.shape) - r) / (np.abs(r).max() + 1e-12)
        print(f"d {n}: max {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e} of the largest entry {np.abs(r).max():.3e}")
    for n, r in ref.items():
        r = r.numpy()
        err = np.abs(grads[n].cpu().numpy().reshape(r.shape) - r) / (np.abs(r).max() + 1e-12)
        assert err.max() < 5e-3 and np.sqrt((err ** 2).mean()) < 5e-4, (n, err.max())


def test_fitter_graph_follows_the_principal_table(tables):
    """Three fit_step_graph iterations equal three eager ones (compared as test_graph_captured_step_equals_eager_step does: losses
    rtol 2e-4, parameters to 2e-4, fov to 5e-3); set_cameras with another principal table drops the captured graph and the next
    iteration follows the new cameras."""
    from smilify_amd import synthetic

    t = tables("synthetic")
    w, wt = synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL
    fe, fg = _fit_problem(t, 2), _fit_problem(t, 2)
    for f in (fe, fg):
        f.begin_stage(synthetic.STAGE1_LR)

    def both():
        a, b = fe.fit_step(w, wt).clone(), fg.fit_step_graph(w, wt).clone()
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=2e-4, atol=1e-6)
        for n in PARAMS:
            np.testing.assert_allclose(getattr(fg, n).detach().cpu().numpy(), getattr(fe, n).detach().cpu().numpy(), atol=5e-3 if n == "fov" else 2e-4, err_msg=n)
        return a

    for _ in range(3):
        last = both()
    first = fg._graph["graph"]
    cam = fg.renderer.cameras
    for f in (fe, fg):
        f.set_cameras(cam.R, cam.T, principal_point=FIT_PP + torch.tensor([0.3, -0.25]))
    assert fg._graph is None
    moved = both()
    assert fg._graph["graph"] is not first
    assert float(moved[0]) > 2.0 * float(last[0])  # the joints are now ~9 px off their targets: the 2-D term sees the new cameras
    for f in (fe, fg):  # in place: the captured launches read the same buffer, no new capture
        f.renderer.cameras.principal_point -= torch.tensor([0.3, -0.25], device=DEV)
    second = fg._graph["graph"]
    back = both()
    assert fg._graph["graph"] is second and float(back[0]) < 0.75 * float(moved[0])
    with pytest.raises(NotImplementedError, match="gradient"):
        fe.set_cameras(cam.R, cam.T, principal_point=FIT_PP.clone().requires_grad_())


def test_cached_epoch_sees_an_in_place_edit_of_the_principal_table(tables):
    """forward() serves the windows of an epoch from one cached evaluation; an in-place edit of renderer.cameras.principal_point
    must drop it: the next windows equal those of a fresh fitter with the edited table (same kernels on the same inputs: 1e-5, as
    test_invalidate_targets_drops_the_cached_epoch) and not the cached ones."""
    from smilify_amd import synthetic

    t = tables("synthetic")
    w = synthetic.STAGE1_WEIGHTS

    def windows(f):
        return [float(f([j], w, 1)[0]) for j in range(2)]

    f = _fit_problem(t, 1)
    stale = windows(f)
    assert f._epoch is not None and f._epoch["served"] >= 1
    assert windows(f) == stale  # (served from the cache)
    f.renderer.cameras.principal_point[:, 0] += 0.2
    got = windows(f)
    fresh = _fit_problem(t, 1, pp=f.renderer.cameras.principal_point.cpu().clone())
    want = windows(fresh)
    print(f"stale {stale} after the edit {got} fresh {want}")
    for g, x, s in zip(got, want, stale):
        assert abs(g - x) <= 1e-5 * abs(x) and abs(g - s) > 1e-3 * abs(s)


def test_round_trip_through_triangulation_with_principal_points(golden):
    """The STICK fixture joints -> a ring of 4 cameras with principal offsets (Renderer, joints_only) ->
    projection_matrix_from_fov_camera(principal_point=) -> triangulate_all -> the joints again within 2e-4, the fp32 figure of
    test_projection_round_trip_recovers_the_reference_fixture_joints."""
    from smilify_amd import triangulate
    from smilify_amd.cameras import look_at_view_transform
    from smilify_amd.p3d_renderer import Renderer

    S, V = 512, 4
    joints = torch.from_numpy(golden("lbs_stick")["fixture_joints"]).float().to(DEV)  # (2, 55, 3)
    B, J = joints.shape[0], joints.shape[1]
    az = torch.linspace(0, 360, V + 1)[:V]
    Rm, T = look_at_view_transform(3.0, torch.full_like(az, 15.0), az)
    fov = torch.full((V,), 60.0)
    pp = torch.tensor([[0.3, -0.2], [-0.25, 0.15], [0.1, 0.35], [-0.4, -0.3]])
    rend = Renderer(S, DEV, views=V)
    rend.set_camera_parameters(Rm, T, fov, principal_point=pp)
    _, yx = rend(joints, joints, None, joints_only=True)
    yx = yx.cpu().numpy().astype(np.float64).reshape(B, V, J, 2)
    cams = {f"view{v}": dict(P=triangulate.projection_matrix_from_fov_camera(Rm[v], T[v], 60.0, 1.0, S, principal_point=pp[v])) for v in range(V)}
    coords = {f"view{v}": yx[:, v, :, ::-1].copy() for v in range(V)}  # (x, y)
    scores = {f"view{v}": np.ones((B, J)) for v in range(V)}
    tracks, stats = triangulate.triangulate_all(cams, coords, scores, B, J, reproj_threshold=2.0, verbose=False)
    assert stats["triangulated"] == B * J and stats["mean_views_used"] == V
    err = np.linalg.norm(tracks[:, 0] - joints.cpu().numpy(), axis=-1)
    centred = {f"view{v}": dict(P=triangulate.projection_matrix_from_fov_camera(Rm[v], T[v], 60.0, 1.0, S)) for v in range(V)}
    off, _ = triangulate.triangulate_all(centred, coords, scores, B, J, reproj_threshold=1e9, verbose=False)
    err_off = np.linalg.norm(off[:, 0] - joints.cpu().numpy(), axis=-1)
    print(f"round trip: max {err.max():.3e} mean {err.mean():.3e}; with the offsets dropped from P: max {np.nanmax(err_off):.3e}")
    assert err.max() < 2e-4, err.max()
    assert not np.nanmax(err_off) < 1e-2  # (the offsets matter: matrices without them put the joints elsewhere)
