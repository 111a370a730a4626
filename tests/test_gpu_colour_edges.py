"""GPU tests of the colour (HardPhong) path at its edges (``pytest -m gpu``): ``engine.render_colour`` against the float64 restatement
(tests/shade_ref.py) on the purpose-built scenes of tests/colour_cases.py - partial tiles, the unbinned loop (by overflow and by size),
exact depth ties, lists of 64 / 65 / 128 / 129 entries in both depth orders, both kinds of cut face in every corner position, the
specular lobe, back faces, degenerate normals, camera tables of 1 / views / N rows and batches cut into several launches.
tests/test_colour_cpu.py shows from the restatement alone that every scene reaches its branch.

Conditions: no ``pix_to_face`` mismatch outside the restatement's ``unsure_face`` pixels (declared exact ties are compared: the lower id
must win), mismatches inside at most 1e-3 N S^2, colour within 2e-4 wherever the face agrees, background exactly 1, two calls
bit-identical.  The shading scenes add the float32 yardstick: GPU error <= max(4 x the error of the same formulas in numpy float32 at
the restatement's barycentrics, 2^-21).  Every test prints the numbers of compared and excluded pixels and the largest colour error."""
import numpy as np
import pytest
import torch

import colour_cases as cc
import shade_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _render(s, frames=None, ndc=True):
    """(image, pix_to_face) of the scene's frames (default: all) as numpy arrays, from the scene's NDC vertices or (``ndc=False``)
    from the engine's own projection of the world vertices."""
    from smilify_amd import engine
    from smilify_amd.p3d_renderer import _MeshTopology

    if "dm" not in s.__dict__:
        s.dm = _MeshTopology(s.faces, s.verts_world.shape[1], torch.device(DEV)).dm
    frames = range(s.verts_world.shape[0]) if frames is None else frames
    images = [f * s.views + v for f in frames for v in range(s.views)]
    dev = lambda a, idx=None: None if a is None else torch.from_numpy(a if idx is None or len(a) != s.N else a[idx]).to(DEV).contiguous()  # noqa: E731
    cams = engine.CameraSet(dev(s.R, images), dev(s.T, images), dev(s.fov, images), dev(s.aspect, images), s.views, s.S)
    img, p2f = engine.render_colour(s.dm, cams, dev(s.verts_world[list(frames)]), cc.RGB,
                                    verts_ndc=dev(s.verts_ndc[images]) if ndc else None, want_pix_to_face=True)
    torch.cuda.synchronize()
    assert img.shape == (len(images), 3, s.S, s.S) and img.dtype == torch.float32 and p2f.shape == (len(images), s.S, s.S)
    return img.cpu().numpy(), p2f.cpu().numpy()


def _check(name, yardstick=False):
    """Render the scene twice and judge it; returns ``(image, pix_to_face)``."""
    s, ref = cc.get(name), cc.reference(name)
    img, p2f = _render(s)
    again = _render(s)
    assert np.array_equal(img, again[0]) and np.array_equal(p2f, again[1])   # two calls: bit-identical
    assert np.isfinite(img).all()
    bad = hits = out = 0
    err = err32 = 0.0
    for n, r in enumerate(ref):
        b, h, e, agree = cc.compare_image(img[n], p2f[n], r.image, r.pix_to_face, r.unsure, s.F, r.unsure_face, r.excluded)
        bad, hits, err, out = bad + b, hits + h, max(err, e), out + int((r.unsure | r.excluded).sum())
        if s.dup_of is not None:  # exact ties are compared, and decided for the lower id
            assert np.array_equal(p2f[n][r.tie & ~r.unsure_face], r.pix_to_face[r.tie & ~r.unsure_face])
        if agree.any():
            err32 = max(err32, float(np.abs(r.image32[:, agree] - r.image[:, agree]).max()))
    print(f"{name}: compared {hits} hit pixels, {out} excluded as unsure, {bad} mismatches inside them, colour error {err:.3e} "
          f"(float32 evaluation {err32:.3e})")
    assert bad <= 1e-3 * s.N * s.S * s.S, bad
    if yardstick:
        assert err <= max(4.0 * err32, 2.0 ** -21), (err, err32)
    return img, p2f


@pytest.mark.parametrize("S", cc.PARTIAL_SIZES)
def test_partial_tiles(S):
    """S no multiple of 8: hits in the last, partial tile row and column; the whole output is compared."""
    name = f"partial{S}"
    _, p2f = _check(name)
    r = cc.reference(name)[0]
    ok = (p2f[0] >= 0) & (p2f[0] == r.pix_to_face) & ~r.unsure
    assert ok[:, 8 * (S // 8):].any() and ok[8 * (S // 8):].any()


def test_fallback_by_overflow():
    """An image whose tile lists do not fit (unbinned loop) beside a binned one in one launch; the binned one equals its own render."""
    s = cc.get("overflow")
    img, p2f = _check("overflow")
    alone = _render(s, frames=[1])
    assert np.array_equal(img[1], alone[0][0]) and np.array_equal(p2f[1], alone[1][0])


@pytest.mark.parametrize("S", [520, 516])
def test_fallback_by_size(S):
    """More than 4096 tiles: never binned (516: with partial tiles as well)."""
    _check(f"size{S}")


@pytest.mark.parametrize("name", cc.TIES)
def test_exact_ties(name):
    """Bit-identical copies of every face: the lower id wins on every hit pixel, whichever copy arrives first - in one batch, in
    different batches of a tile, with the table shuffled, and in different 64-face groups of the unbinned loop."""
    _, p2f = _check(name)
    s = cc.get(name)
    for n, r in enumerate(cc.reference(name)):
        sure = r.tie & ~r.unsure_face
        assert sure.sum() > 50 and np.array_equal(s.dup_of[p2f[n][sure]], p2f[n][sure])


@pytest.mark.parametrize("name", cc.STACKS)
def test_batch_edges_and_rejection_order(name):
    """64, 65, 128, 129 faces on one tile, near to far and far to near: the nearest wins on every pixel of the tile; with a nearest
    face that covers only a corner of it, the faces behind are still drawn on the rest."""
    _, p2f = _check(name)
    tx, ty = cc.STACK_TILE
    assert np.array_equal(p2f[0][ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], cc.reference(name)[0].pix_to_face[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8])


def test_cut_faces_in_every_corner_position():
    """One and two vertices behind z_clip, in each of the three corners: at least 50 compared pixels per kind lie on a front part.
    Pixels that only hang between the two parts of one face are compared too (either part is the same face)."""
    _, p2f = _check("cuts")
    s = cc.get("cuts")
    for n, r in enumerate(cc.reference("cuts")):
        ok = (p2f[n] == r.pix_to_face) & (r.part >= 0) & ~r.unsure
        for kind in (1, 2):
            assert (ok & np.isin(r.pix_to_face, np.flatnonzero(s.info["n_behind"] == kind))).sum() >= 50


@pytest.mark.parametrize("name", cc.SHADING)
def test_shading_terms(name):
    """The specular lobe (peak and flank), back faces (ambient only, no specular although v.r > 0) and degenerate normals (a vertex of
    no face, faces without area, opposite normals interpolating to zero), against the float32 yardstick."""
    img, p2f = _check(name, yardstick=True)
    if name == "degenerate":
        assert not np.isin(p2f, cc.get(name).info["no_area"]).any()


@pytest.mark.parametrize("rows", ["N", "1", "views"])
def test_camera_tables_and_slicing(rows, monkeypatch):
    """3 frames x 2 views through camera tables of N, 1 and ``views`` rows; cut into launches of one frame the result is the same to
    the bit; and the engine's own projection of the world vertices gives the image the given NDC gives."""
    from smilify_amd import engine

    name = f"cameras_{rows}"
    s = cc.get(name)
    whole = _check(name)
    # the engine's projection differs from the scene's in the last bits: judged by the restatement of its own NDC vertices
    cams = engine.CameraSet(*[torch.from_numpy(a).to(DEV) for a in (s.R, s.T, s.fov, s.aspect)], s.views, s.S)
    ndc = engine.project(cams, torch.from_numpy(s.verts_world).to(DEV), want_yx=False)[0].double().cpu().numpy()
    np.testing.assert_allclose(ndc, s.verts_ndc, rtol=1e-5, atol=1e-6)
    own = _render(s, ndc=False)
    for n in range(s.N):
        ref, rp, unsure = shade_ref.render_colour(s.verts_world[n // s.views], ndc[n], s.faces, s.R[n % len(s.R)], s.T[n % len(s.T)], cc.RGB, s.S)
        cc.compare_image(own[0][n], own[1][n], ref, rp, unsure, s.F)
    monkeypatch.setattr(engine, "MAX_COLOUR_WORKSPACE_BYTES", 1)
    for ndc in (True, False):
        sliced = _render(s, ndc=ndc)
        want = whole if ndc else own
        assert np.array_equal(sliced[0], want[0]) and np.array_equal(sliced[1], want[1])
