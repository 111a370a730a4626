"""GPU tests of the colour (HardPhong) path (``pytest -m gpu``): ``engine.render_colour`` / ``Renderer(colour=True)`` /
``FitterConfig.RENDER_COLOUR`` against the float64 restatement in tests/shade_ref.py, on posed templates of the three models: what real
meshes exercise, the public entry points and the full sizes.  The branches real meshes do not reach (partial tiles, the unbinned loop,
exact ties, batch edges, cut faces corner by corner, the shading terms one by one, camera tables and slicing) are pinned on purpose-built
scenes in tests/test_gpu_colour_edges.py."""
import numpy as np
import pytest
import torch

import colour_cases
import shade_ref
from oracle import render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB = [0.0, 172.0 / 255.0, 223.0 / 255.0]


def _posed(t, frames, seed, radius=1.0):
    """``frames`` copies of the template, centred, scaled to ``radius`` and turned by a random rotation each."""
    g = torch.Generator().manual_seed(seed)
    v = torch.from_numpy(np.asarray(t.v_template, np.float32))
    v = v - v.mean(0)
    v = v * (radius / float(v.norm(dim=1).max()))
    out = []
    for _ in range(frames):
        q = torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)
        a, b, c, d = q.tolist()
        R = torch.tensor([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                          [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                          [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
        out.append(v @ R.T + 0.05 * torch.randn(3, generator=g))
    return torch.stack(out).contiguous()


def _cams(views, frames, S, dist=2.7, aspect=None, per_image_fov=True):
    from smilify_amd import engine

    R, T = render_ref.look_at_view_transform(dist, torch.linspace(-10, 25, views), torch.linspace(0, 140, views))
    N = frames * views
    fov = torch.linspace(45.0, 70.0, N) if per_image_fov else torch.tensor([60.0])
    asp = None if aspect is None else torch.full((N,), float(aspect))
    return engine.CameraSet(R.to(DEV).contiguous(), T.to(DEV).contiguous(), fov.to(DEV).contiguous(),
                            None if asp is None else asp.to(DEV).contiguous(), views, S)


def _check(verts, cams, t, images=None, dm=None):
    """render_colour against shade_ref on the given images; returns the numbers of unsure and compared pixels."""
    from smilify_amd import engine

    dm = dm or engine.DeviceModel(t, DEV)
    verts = verts.to(DEV)
    ndc, _ = engine.project(cams, verts, want_yx=False)
    img, p2f = engine.render_colour(dm, cams, verts, RGB, verts_ndc=ndc, want_pix_to_face=True)
    torch.cuda.synchronize()
    N = ndc.shape[0]
    S = cams.S
    assert img.shape == (N, 3, S, S) and img.dtype == torch.float32 and p2f.shape == (N, S, S)
    ndc_h, img_h, p2f_h, vw = ndc.double().cpu().numpy(), img.cpu().numpy(), p2f.cpu().numpy(), verts.cpu().numpy()
    Rh, Th = cams.R.cpu().numpy(), cams.T.cpu().numpy()
    bad = hits = 0
    for n in (range(N) if images is None else images):
        R, T = Rh[n % Rh.shape[0]], Th[n % Th.shape[0]]
        ref, rp, unsure = shade_ref.render_colour(vw[n // cams.views], ndc_h[n], t.faces, R, T, RGB, S)
        b, h, _, _ = colour_cases.compare_image(img_h[n], p2f_h[n], ref, rp, unsure, t.F)
        bad += b
        hits += h
    n_img = N if images is None else len(images)
    assert bad <= 1e-3 * n_img * S * S, bad
    return bad, hits


@pytest.mark.parametrize("model", ["synthetic", "stick"])
@pytest.mark.parametrize("S", [64, 128])
def test_render_colour_matches_the_restatement(tables, model, S):
    """3 frames x 2 views, per-image fov, non-square aspect ratio."""
    t = tables(model)
    verts = _posed(t, 3, seed=S + len(model))
    cams = _cams(2, 3, S, aspect=1.3)
    _, hits = _check(verts, cams, t)
    assert hits > 100  # (the stick insect covers little of the image)


def test_render_colour_square_and_shared_fov(tables):
    t = tables("stick")
    _, hits = _check(_posed(t, 2, seed=5), _cams(1, 2, 64, per_image_fov=False), t)
    assert hits > 0


def test_faces_cut_at_z_clip(tables):
    """The camera inside the mesh: faces crossing z_clip = znear / 2 are drawn by their front parts, reported as their original
    face (ids < F), ties resolved by (depth, parent face, part)."""
    t = tables("synthetic")
    verts = _posed(t, 2, seed=9, radius=1.0)
    cams = _cams(2, 2, 64, dist=0.35, aspect=0.9)
    from smilify_amd import engine

    ndc, _ = engine.project(cams, verts.to(DEV), want_yx=False)
    z = ndc[..., 2].cpu().numpy()
    cut = sum(int(((z[n][t.faces] < shade_ref.Z_CLIP).sum(1) % 3 != 0).sum()) for n in range(z.shape[0]))
    assert cut > 0
    _, hits = _check(verts, cams, t)
    assert hits > 0


def test_full_size_stick_4096_images_and_mouse_512(tables):
    from smilify_amd import engine

    t = tables("stick")
    dm = engine.DeviceModel(t, DEV)
    verts = _posed(t, 4096, seed=1).to(DEV)
    cams = _cams(1, 4096, 256, per_image_fov=False)
    _check(verts, cams, t, images=[0, 1111, 2222, 4095], dm=dm)
    tm = tables("mouse")
    vm = _posed(tm, 2, seed=2)
    _check(vm, _cams(18, 2, 512, per_image_fov=False), tm, images=[0, 25])


def test_two_calls_are_bit_identical(tables):
    from smilify_amd import engine

    t = tables("stick")
    dm = engine.DeviceModel(t, DEV)
    verts = _posed(t, 64, seed=3).to(DEV)
    cams = _cams(2, 64, 128)
    a, pa = engine.render_colour(dm, cams, verts, RGB, want_pix_to_face=True)
    b, pb = engine.render_colour(dm, cams, verts, RGB, want_pix_to_face=True)
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_renderer_colour_opt_in(tables):
    from smilify_amd.p3d_renderer import Renderer

    t = tables("stick")
    S = 64
    r = Renderer(S, DEV, colour=True)
    assert r.mesh_color.shape == (1, 1, 3)
    faces = torch.from_numpy(t.faces.astype(np.int64)).to(DEV)[None].expand(2, -1, -1)
    v0 = _posed(t, 2, seed=4).to(DEV)
    pts = v0[:, :10].clone()
    v1 = v0.clone().requires_grad_(True)
    sil1, proj1 = r(v1, pts, faces)
    sil1.sum().backward()
    v2 = v0.clone().requires_grad_(True)
    sil2, proj2, col = r(v2, pts, faces, render_texture=True)
    sil2.sum().backward()
    assert torch.equal(sil1, sil2) and torch.equal(proj1, proj2)
    # (a call this small accumulates the silhouette gradient with float atomics: equal up to their order, as without colour)
    torch.testing.assert_close(v2.grad, v1.grad, rtol=0.0, atol=1e-5 * float(v1.grad.abs().max()))
    assert col.shape == (2, 3, S, S) and not col.requires_grad
    assert torch.equal(col, r.render_colour(v0, faces))
    with pytest.raises(NotImplementedError):
        Renderer(S, DEV)(v0, pts, faces, render_texture=True)


def test_fitter_render_colour_panels(tables, monkeypatch):
    """RENDER_COLOUR = True: the render panel of generate_visualization is the uint8 of render_colour for that frame.  With the switch
    off the same fitter's collage is what a default fitter produces, byte for byte."""
    from smilify_amd import synthetic
    from smilify_amd.config import FitterConfig

    t = tables("synthetic")
    N, W, S = 3, 2, 40

    def run(model):
        calls = []

        class Exporter:
            stage_id, epoch_name = 1, "0"

            def export(self, collage_np, batch_id, global_id, img_parameters, vertices, faces, img_idx=0, epoch=None):
                calls.append((collage_np, vertices[batch_id].detach().clone()))

        model.generate_visualization(Exporter())
        return calls

    default = run(synthetic.make_problem(t, N, 1, S, DEV, radius=2.2, seed=3, window=W))
    orig = FitterConfig.from_tables

    def with_colour(*a, **k):
        cfg = orig(*a, **k)
        cfg.RENDER_COLOUR = True
        return cfg
    monkeypatch.setattr(FitterConfig, "from_tables", staticmethod(with_colour))
    model = synthetic.make_problem(t, N, 1, S, DEV, radius=2.2, seed=3, window=W)
    assert model.renderer.colour
    coloured = run(model)
    faces = model.smal_model.faces[None]
    for (collage, v), (plain, _) in zip(coloured, default):
        want = model.renderer.render_colour(v[None].contiguous(), faces)[0].clamp(0.0, 1.0).permute(1, 2, 0).cpu().numpy()
        np.testing.assert_array_equal(collage[:, S:2 * S], (want * 255.0).astype(np.uint8))
        np.testing.assert_array_equal(collage[:, 3 * S:4 * S], plain[:, 3 * S:4 * S])  # silhouette agreement panel unchanged
        assert not np.array_equal(collage[:, S:2 * S], plain[:, S:2 * S])
    model.renderer.colour = False
    for (collage, _), (plain, _) in zip(run(model), default):
        np.testing.assert_array_equal(collage, plain)
