"""GPU tests of ``engine.render_fragments`` (``pytest -m gpu``): the hard rasteriser's pix_to_face / zbuf / bary / dist against the float64
restatement (tests/shade_ref.py, tests/fragments_ref.py) on edge scenes of tests/colour_cases.py - partial tiles, the unbinned loop, exact
depth ties, 129 entries far to near, both kinds of cut face, degenerate faces, camera tables of N / 1 / views rows.

Conditions: ``pix_to_face`` by ``colour_cases.compare_image``'s rule (no mismatch outside ``unsure_face``, declared ties to the lower id,
mismatches inside at most 1e-3 N S^2); where the face agrees and the pixel is not ``unsure``, the errors of zbuf, bary and dist against
float64 at most max(4 x the error of the same formulas in numpy float32 on that scene, floor), floor = 2^-21 of the scene's largest depth
(zbuf, dist) or 2^-21 (bary): the rule of tests/test_gpu_colour_edges.py.  Background exactly -1 / -1 / -1 / +inf, barycentrics of a hit sum
to 1 within 1e-6, two calls bit-identical.  tests/test_colour_cpu.py::test_scene_exclusions_stay_under_two_percent bounds what ``unsure``
leaves out of each scene.  Every case prints the compared and excluded counts and the largest errors."""
import ctypes

import numpy as np
import pytest
import torch

import colour_cases as cc
import fragments_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup(s, frames=None):
    """(device model, cameras, world vertices, NDC vertices, images) of the scene's frames (default: all) on the GPU."""
    from smilify_amd import engine
    from smilify_amd.p3d_renderer import _MeshTopology

    if "dm" not in s.__dict__:
        s.dm = _MeshTopology(s.faces, s.verts_world.shape[1], torch.device(DEV)).dm
    frames = range(s.verts_world.shape[0]) if frames is None else frames
    images = [f * s.views + v for f in frames for v in range(s.views)]
    dev = lambda a, idx=None: None if a is None else torch.from_numpy(a if idx is None or len(a) != s.N else a[idx]).to(DEV).contiguous()  # noqa: E731
    cams = engine.CameraSet(dev(s.R, images), dev(s.T, images), dev(s.fov, images), dev(s.aspect, images), s.views, s.S)
    return s.dm, cams, dev(s.verts_world[list(frames)]), dev(s.verts_ndc[images]), images


def _fragments(s, want=None):
    from smilify_amd import engine

    dm, cams, world, ndc, images = _setup(s)
    fr = engine.render_fragments(dm, cams, world, verts_ndc=ndc, want=want or engine.FRAGMENT_OUTPUTS)
    torch.cuda.synchronize()
    return engine.Fragments(*[None if t is None else t.cpu().numpy() for t in fr])


@pytest.mark.parametrize("name", FR.FRAGMENT_SCENES)
def test_fragments_on_edge_scenes(name):
    s, ref = cc.get(name), FR.reference(name)
    fr, again = _fragments(s), _fragments(s)
    N, S = s.N, s.S
    assert fr.pix_to_face.shape == (N, S, S) and fr.pix_to_face.dtype == np.int32
    assert fr.zbuf.shape == (N, S, S) and fr.bary.shape == (N, S, S, 3) and fr.dist.shape == (N, S, S)
    assert fr.zbuf.dtype == fr.bary.dtype == fr.dist.dtype == np.float32
    for a, b in zip(fr, again):                                     # two calls: bit-identical
        assert np.array_equal(a, b)
    bad = hits = out = 0
    ez = eb = ed = esum = 0.0
    for n, r in enumerate(ref):
        p2f = fr.pix_to_face[n]
        diff = p2f != r.pix_to_face
        assert not (diff & ~r.unsure_face).any(), (np.argwhere(diff & ~r.unsure_face)[:8], p2f[diff & ~r.unsure_face][:8])
        assert p2f.max() < s.F and p2f.min() >= -1
        if s.dup_of is not None:                                    # exact ties are compared, and decided for the lower id
            sure = r.tie & ~r.unsure_face
            assert np.array_equal(p2f[sure], r.pix_to_face[sure])
        bad, out = bad + int(diff.sum()), out + int(r.unsure.sum())
        bg = p2f < 0                                                # background: exactly -1 / -1 / +inf
        assert (fr.zbuf[n][bg] == -1.0).all() and (fr.bary[n][bg] == -1.0).all() and np.isposinf(fr.dist[n][bg]).all()
        hit = ~bg
        assert np.isfinite(fr.zbuf[n][hit]).all() and np.isfinite(fr.bary[n][hit]).all() and np.isfinite(fr.dist[n][hit]).all()
        if hit.any():
            esum = max(esum, float(np.abs(fr.bary[n][hit].astype(np.float64).sum(-1) - 1.0).max()))
        ok = ~diff & (r.pix_to_face >= 0) & ~r.unsure
        hits += int(ok.sum())
        if ok.any():
            ez = max(ez, float(np.abs(fr.zbuf[n][ok] - r.zbuf[ok]).max()))
            eb = max(eb, float(np.abs(fr.bary[n][ok] - r.bary[ok]).max()))
            ed = max(ed, float(np.abs(fr.dist[n][ok] - r.dist[ok]).max()))
    yz, yb, yd, zmax, dmax = FR.yardstick(name)
    bz, bb, bd = max(4.0 * yz, FR.FLOOR * zmax), max(4.0 * yb, FR.FLOOR), max(4.0 * yd, FR.FLOOR * dmax)
    print(f"{name}: compared {hits} hit pixels, {out} excluded as unsure, {bad} face mismatches inside them; errors (float32 evaluation, bound) "
          f"zbuf {ez:.3e} ({yz:.3e}, {bz:.3e}) bary {eb:.3e} ({yb:.3e}, {bb:.3e}) dist {ed:.3e} ({yd:.3e}, {bd:.3e}); |sum bary - 1| {esum:.3e}")
    assert hits > 0
    assert bad <= 1e-3 * N * S * S, bad
    assert esum <= 1e-6, esum
    assert ez <= bz, (ez, yz, bz)
    assert eb <= bb, (eb, yb, bb)
    assert ed <= bd, (ed, yd, bd)


def test_fragments_optional_outputs():
    """Each output alone equals the same output of the full call to the bit; without ``dist`` the ABI takes verts_world = NULL (and
    cameras without tables)."""
    from smilify_amd import _lib, engine

    s = cc.get("cuts")
    full = _fragments(s)
    for k, name in enumerate(engine.FRAGMENT_OUTPUTS):
        alone = _fragments(s, want=(name,))
        assert [t is not None for t in alone] == [j == k for j in range(4)]
        assert np.array_equal(alone[k], full[k]), name
    dm, cams, _, ndc, _ = _setup(s)
    lib = _lib.load()
    p2f = torch.empty(s.N, s.S, s.S, dtype=torch.int32, device=DEV)
    zbuf = torch.empty(s.N, s.S, s.S, dtype=torch.float32, device=DEV)
    bary = torch.empty(s.N, s.S, s.S, 3, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.smil_fragments_workspace_bytes(dm.handle, s.N, s.S)), dtype=torch.uint8, device=DEV)
    assert 0 < ws.numel() <= int(lib.smil_colour_workspace_bytes(dm.handle, s.N, s.S)) - s.N * dm.V * 3 * 4  # the setup's tables, no normals
    c = _lib.Cameras()
    c.N, c.views, c.S = s.N, s.views, s.S   # (no camera tables: only dist reads them)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.smil_render_fragments(dm.handle, ctypes.byref(c), None, ptr(ndc), ptr(p2f), ptr(zbuf), ptr(bary), None, ptr(ws), stream))
    torch.cuda.synchronize()
    assert np.array_equal(p2f.cpu().numpy(), full.pix_to_face) and np.array_equal(zbuf.cpu().numpy(), full.zbuf)
    assert np.array_equal(bary.cpu().numpy(), full.bary)
    # dist without verts_world, and no output at all, are refused
    assert lib.smil_render_fragments(dm.handle, ctypes.byref(c), None, ptr(ndc), None, None, None, ptr(zbuf), ptr(ws), stream) == -1
    assert lib.smil_render_fragments(dm.handle, ctypes.byref(c), None, ptr(ndc), None, None, None, None, ptr(ws), stream) == -1
    with pytest.raises(ValueError):
        _fragments(s, want=("depth",))


@pytest.mark.parametrize("name", ["cuts", "overflow"])
def test_fragments_match_colour_pix_to_face(name):
    from smilify_amd import engine

    s = cc.get(name)
    dm, cams, world, ndc, _ = _setup(s)
    _, p2f = engine.render_colour(dm, cams, world, cc.RGB, verts_ndc=ndc, want_pix_to_face=True)
    fr = engine.render_fragments(dm, cams, world, verts_ndc=ndc, want=("pix_to_face",))
    torch.cuda.synchronize()
    assert torch.equal(p2f, fr.pix_to_face) and (p2f >= 0).any()


def test_fragments_slicing_and_renderer(monkeypatch):
    """3 frames x 2 views cut into launches of one frame give the whole batch's bits (camera tables of N rows follow the slice), and
    ``Renderer.render_fragments`` / ``render_depth`` are the engine's outputs of the renderer's own projection."""
    from smilify_amd import engine
    from smilify_amd.p3d_renderer import Renderer

    s = cc.get("cameras_N")
    whole = _fragments(s)
    monkeypatch.setattr(engine, "MAX_IMAGES_PER_LAUNCH", s.views)
    for a, b in zip(whole, _fragments(s)):
        assert np.array_equal(a, b)
    monkeypatch.undo()
    r = Renderer(s.S, DEV, views=s.views)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    r.set_camera_parameters(t(s.R), t(s.T), t(s.fov), t(s.aspect))
    verts, faces = t(s.verts_world), t(s.faces)[None].expand(s.verts_world.shape[0], -1, -1)
    fr = r.render_fragments(verts, faces)
    ndc = engine.project(r._camera_set(), verts, want_yx=False)[0]
    own = engine.render_fragments(s.dm, r._camera_set(), verts, verts_ndc=ndc)
    for a, b in zip(fr, own):
        assert torch.equal(a, b)
    assert torch.equal(r.render_depth(verts, faces), fr.zbuf) and torch.equal(r.render_depth(verts, faces, kind="distance"), fr.dist)
    hit = fr.pix_to_face >= 0
    assert hit.any() and (fr.dist[hit] >= fr.zbuf[hit] * (1.0 - 1e-6)).all()   # the distance to the centre is no less than the view depth
    with pytest.raises(ValueError):
        r.render_depth(verts, faces, kind="disparity")
