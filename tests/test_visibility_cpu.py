"""CPU checks of what the fragment and depth-visibility GPU tests are judged by (tests/fragments_ref.py): the visibility restatement
reproduces the reference's recorded answers (tests/golden/visibility_ref.npz, written by tests/golden/make_visibility_fixture.py from
smal_fitter/Unreal2Pytorch3D.py:664-760) exactly while a float32 evaluation of the same rules does not, the float32 yardstick of the
fragment outputs is usable on every scene, and the model scene of ``Renderer.keypoint_visibility`` keeps its margins - so that the GPU
tests leave nothing out."""
import os
import re

import numpy as np
import pytest
import torch

import fragments_ref as FR
from conftest import GOLDEN, REPO

GROUPS, NEIGHBORHOODS = ("a", "b"), (0, 1, 2)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "visibility_ref.npz"))


def case(fx, g, h):
    return {k: fx[f"{g}_h{h}_{k}"] for k in ("norm", "points", "camera", "vis_in", "vis_out", "surface")}


def test_exports_are_declared_exported_and_bound():
    from smilify_amd import _lib

    header = open(os.path.join(REPO, "include", "smilfit.h")).read()
    for name in ("smil_fragments_workspace_bytes", "smil_render_fragments", "smil_depth_visibility"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert len(lib.smil_render_fragments.argtypes) == 10 and len(lib.smil_depth_visibility.argtypes) == 16
    assert lib.smil_fragments_workspace_bytes(None, 1, 64) == 0
    assert lib.smil_render_fragments(*[None] * 10) == -1
    assert b"smil_render_fragments" in lib.smil_last_error()
    # the half-window is checked before anything is launched
    for h in (-1, 9):
        assert lib.smil_depth_visibility(None, 0, 1, 0.0, 1, 4, 4, None, None, 1, None, 0.0, h, None, None, None) == -1
        assert b"neighborhood" in lib.smil_last_error()
    assert b"0.5" in lib.smil_version() and b"fragments" in lib.smil_version()


def test_fixture_holds_the_cases_it_promises(fixture):
    """Image sizes, the skipped kinds, bytes 0 and 255, keypoints within 1e-6 of the threshold on either side and none within 1e-12."""
    assert fixture["a_depth"].shape == (3, 12, 20, 4) and fixture["b_depth"].shape == (3, 16, 16, 1)
    total = 0
    for g in GROUPS:
        depth, tol = fixture[f"{g}_depth"], float(fixture[f"{g}_tolerance"])
        assert (depth[..., 0] == 0).any(-1).any(-1).all() and (depth[..., 0] == 255).any(-1).any(-1).all()
        for h in NEIGHBORHOODS:
            c = case(fixture, g, h)
            n = c["norm"]
            total += c["vis_in"].size
            assert (n == 0.0).any() and (n == 1.0).any() and (n < 0.0).any() and (n > 1.0).any() and np.isnan(n).any()
            assert np.isnan(c["points"]).any() and (c["vis_in"] == 0.0).any()
            d = FR.point_distances(c["points"], c["camera"])
            with np.errstate(invalid="ignore"):
                rel = (d - (c["surface"] + tol)) / (c["surface"] + tol)
            assert ((rel > 0) & (rel < 1.5e-6)).sum() >= 5 and ((rel < 0) & (rel > -1.5e-6)).sum() >= 5
            assert not (np.abs(rel) < 1e-12).any()
            assert set(np.unique(c["vis_out"])) <= {0.0, 1.0} and (c["vis_out"] <= c["vis_in"]).all()   # monotone
    assert 200 <= total <= 1000


def test_restatement_reproduces_the_reference(fixture):
    """One image at a time and batched, from the reference's own arguments; float64."""
    for g in GROUPS:
        depth, dmax, tol = fixture[f"{g}_depth"], float(fixture[f"{g}_depth_max"]), float(fixture[f"{g}_tolerance"])
        for h in NEIGHBORHOODS:
            c = case(fixture, g, h)
            vis, surface = FR.refine_visibility_batch(c["vis_in"], c["norm"], c["points"], c["camera"], depth, h, tol, dmax)
            assert np.array_equal(vis, c["vis_out"]) and np.array_equal(surface, c["surface"], equal_nan=True)
            for b in range(len(depth)):
                one, _ = FR.refine_visibility(c["vis_in"][b], c["norm"][b], c["points"][b], c["camera"][b], depth[b], h, tol, dmax)
                assert np.array_equal(one, c["vis_out"][b])
            assert (vis != c["vis_in"]).any()  # (the refinement does something)


def test_float32_evaluation_does_not(fixture):
    """The same rules with the distance, the decoded surface and the comparison in float32 flip keypoints of every case."""
    for g in GROUPS:
        depth, dmax, tol = fixture[f"{g}_depth"], float(fixture[f"{g}_depth_max"]), float(fixture[f"{g}_tolerance"])
        for h in NEIGHBORHOODS:
            c = case(fixture, g, h)
            vis, _ = FR.refine_visibility_batch(c["vis_in"], c["norm"], c["points"], c["camera"], depth, h, tol, dmax, dtype=np.float32)
            assert (vis != c["vis_out"]).sum() >= 1, (g, h)


def test_float_map_of_decoded_bytes_gives_the_recorded_answers(fixture):
    """The float-map form of the rules on the decoded buffer (r / 255 depth_max per pixel, in float64) equals the byte form - the
    minimum commutes with the increasing decoder - and bytes encoded back by ``encode_depth_u8``'s rule are the buffer's own."""
    for g in GROUPS:
        depth, dmax, tol = fixture[f"{g}_depth"], float(fixture[f"{g}_depth_max"]), float(fixture[f"{g}_tolerance"])
        decoded = (depth[..., 0].astype(np.float64) / 255.0) * dmax
        assert np.array_equal(FR.encode_depth_u8(decoded, dmax), depth[..., 0])
        assert FR.encode_depth_u8(np.array([np.inf, 0.0, 2.0 * dmax]), dmax).tolist() == [255, 0, 255]
        for h in NEIGHBORHOODS:
            c = case(fixture, g, h)
            again = FR.encode_depth_u8(decoded, dmax)[..., None]
            vis, surface = FR.refine_visibility_batch(c["vis_in"], c["norm"], c["points"], c["camera"], again, h, tol, dmax)
            assert np.array_equal(vis, c["vis_out"]) and np.array_equal(surface, c["surface"], equal_nan=True)
            vis64, surf64 = FR.refine_visibility_batch(c["vis_in"], c["norm"], c["points"], c["camera"], decoded, h, tol)
            assert np.array_equal(vis64, c["vis_out"]) and np.array_equal(surf64, c["surface"], equal_nan=True)


def test_product_encoder_follows_its_rule():
    """``visibility.encode_depth_u8`` (torch, CPU tensors) against the numpy statement of the rule, ties at .5 and the ends included."""
    from smilify_amd import visibility

    dmax = 437.5
    dist = np.concatenate([np.linspace(-5.0, 2.0 * dmax, 997), (np.arange(256) + 0.5) / 255.0 * dmax, [np.inf, 0.0, dmax]])
    got = visibility.encode_depth_u8(torch.from_numpy(dist.astype(np.float32)), dmax).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, FR.encode_depth_u8(dist.astype(np.float32), dmax))


@pytest.mark.parametrize("name", FR.FRAGMENT_SCENES)
def test_float32_yardstick_is_finite_and_nonzero(name):
    """On every scene of the GPU test the float32 evaluation of zbuf, bary and dist exists on every hit pixel, differs from float64
    (it is a yardstick, not a copy) and by no more than float32 can explain (1e-4 relative: a sanity bound on the restatement, no
    test of the kernel); in float64 the same code reproduces the restatement's own zbuf and barycentrics."""
    import colour_cases as cc

    s = cc.get(name)
    ez, eb, ed, zmax, dmax = FR.yardstick(name)
    print(f"{name}: float32 yardstick zbuf {ez:.3e} (largest {zmax:.3f}), bary {eb:.3e}, dist {ed:.3e} (largest {dmax:.3f})")
    for r in FR.reference(name):
        hit = r.pix_to_face >= 0
        assert np.isfinite(r.zbuf32[hit]).all() and np.isfinite(r.bary32[hit]).all() and np.isfinite(r.dist32[hit]).all()
        assert np.isinf(r.dist[~hit]).all() and np.isfinite(r.dist[hit]).all()
    assert 0.0 < ez <= 1e-4 * zmax and 0.0 < eb <= 1e-4 and 0.0 < ed <= 1e-4 * dmax
    r = FR.reference(name)[0]
    z64, b64 = FR.winner_terms(r.pix_to_face, r.part, s.verts_ndc[0], s.faces, s.S, np.float64)
    hit = r.pix_to_face >= 0
    np.testing.assert_allclose(z64[hit], r.zbuf[hit], rtol=1e-12, atol=0)
    np.testing.assert_allclose(b64[hit], r.bary[hit], rtol=0, atol=1e-12)


def test_model_scene_margins():
    """The scene of test_renderer_keypoint_visibility: every kind of point occurs, every sampled point is at least 1e-3 (relative) from
    its threshold and every projection 0.05 px from a pixel boundary, and no window holds an ``unsure`` pixel."""
    s = FR.visibility_scene()
    rel, px, unsure = FR.visibility_scene_margins(s)
    print(f"model scene: threshold margin {rel:.3e}, pixel margin {px:.3f} px, unsure pixels in windows {unsure}")
    assert rel >= FR.VIS_MARGIN_REL and px >= FR.VIS_MARGIN_PX and unsure == 0
    e, v0 = s.expected, slice(0, None, s.views)           # camera 0 of every frame: the camera the points were placed for
    assert (e[v0, 0] == 1).all() and (e[v0, 1] == 0).all() and (e[v0, 2] == 0).all()      # in front, behind, far surface
    assert (e[v0, 3] == 1).all() and np.isinf(s.surface[v0, 3]).all()                     # beside the silhouette: background
    assert (e[v0, 4] == 1).all() and np.isnan(s.surface[v0, 4]).all()                     # outside the image: not sampled
    assert (e[:, 5] == 0).all() and np.isnan(s.surface[:, 5]).all()                       # visibility 0 coming in
    assert (e[v0, 6] == 1).all() and (e[v0, 7] == 0).all()                                # above the surface, under it
    assert 0 < e.sum() < e.size and (e != s.vis_in).any()
