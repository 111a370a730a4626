"""GPU tests of the depth visibility kernel and the layers above it (``pytest -m gpu``): ``engine.depth_visibility`` and
``visibility.refine_visibility_with_depth`` against the reference's recorded answers (tests/golden/visibility_ref.npz), a float map
against the restatement (tests/fragments_ref.py), ``Renderer.keypoint_visibility`` on the model scene whose margins
tests/test_visibility_cpu.py asserts, and ``SMALFitter.joint_self_occlusion``."""
import os

import numpy as np
import pytest
import torch

import fragments_ref as FR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS, NEIGHBORHOODS = ("a", "b"), (0, 1, 2)


def _case(fx, g, h):
    return {k: fx[f"{g}_h{h}_{k}"] for k in ("norm", "points", "camera", "vis_in", "vis_out", "surface")}


def test_depth_visibility_reference_fixture():
    """The reference's answers, exactly: one image at a time through its own signature (numpy in, numpy out, refined in place), all
    images of a case in one launch (arrays and tensors), and the sampled surface to the bit."""
    from smilify_amd import engine, visibility

    fx = np.load(os.path.join(GOLDEN, "visibility_ref.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    total = 0
    for g in GROUPS:
        depth, dmax, tol = fx[f"{g}_depth"], float(fx[f"{g}_depth_max"]), float(fx[f"{g}_tolerance"])
        H, W = depth.shape[1:3]
        for h in NEIGHBORHOODS:
            c = _case(fx, g, h)
            for b in range(len(depth)):
                vis = c["vis_in"][b].copy()
                back = visibility.refine_visibility_with_depth(vis, c["norm"][b], c["points"][b], c["camera"][b], depth[b], W, H, depth_max_cm=dmax,
                                                               depth_tolerance_cm=tol, depth_neighborhood=h)
                assert back is vis and np.array_equal(vis, c["vis_out"][b]), (g, h, b)
            out = visibility.refine_visibility_with_depth(c["vis_in"], c["norm"], c["points"], c["camera"], depth, W, H, dmax, tol, h)
            assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out, c["vis_out"]), (g, h)
            out_t = visibility.refine_visibility_with_depth(t(c["vis_in"]), t(c["norm"]), t(c["points"]), t(c["camera"]), t(depth), W, H, dmax, tol, h)
            assert out_t.device.type == "cuda" and np.array_equal(out_t.cpu().numpy(), c["vis_out"])
            kp_dist = (t(c["points"]) - t(c["camera"])[:, None]).norm(dim=-1)
            out_e, surface = engine.depth_visibility(t(depth), t(c["norm"]), kp_dist, t(c["vis_in"]), tol, h, depth_max=dmax, want_surface=True)
            assert np.array_equal(out_e.cpu().numpy(), c["vis_out"])
            assert np.array_equal(surface.cpu().numpy().view(np.uint64), c["surface"].view(np.uint64)), (g, h)   # to the bit, NaN included
            total += out.size
    print(f"visibility fixture: {total} keypoints reproduced")
    # the reference's early returns
    c = _case(fx, "a", 1)
    vis = c["vis_in"][0].copy()
    depth = fx["a_depth"]
    for bad in (None, depth[0][..., 0], depth[0][:-1]):
        assert visibility.refine_visibility_with_depth(vis, c["norm"][0], c["points"][0], c["camera"][0], bad, 20, 12) is vis
        assert np.array_equal(vis, c["vis_in"][0])


def test_depth_visibility_float_map():
    """A 9 x 13 float map with +inf background, half-windows 0, 1, 2 and 8 (larger than the map), against the restatement; 9 and -1
    are refused."""
    from smilify_amd import _lib, engine

    rng = np.random.default_rng(3)
    B, H, W, P, tol = 2, 9, 13, 64, 0.25
    depth = rng.uniform(2.0, 6.0, (B, H, W)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.4] = np.inf
    depth[1, 2:7, 3:10] = np.inf                                    # windows of background only
    norm = rng.uniform(-0.05, 1.05, (B, P, 2))
    norm[:, :4] = [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]
    norm[:, 4] = [np.nan, 0.5]
    dist = rng.uniform(1.5, 7.0, (B, P))
    dist[:, 5], dist[:, 6] = np.nan, np.inf
    vis_in = np.ones((B, P), np.float32)
    vis_in[:, 7], vis_in[:, 8] = 0.0, 0.5                          # 0 stays 0; any other value counts as visible and stays itself
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    for h in (0, 1, 2, 8):
        want, want_surface = FR.visibility_rules_batch(vis_in, norm, dist, depth, h, tol)
        got, surface = engine.depth_visibility(t(depth), t(norm), t(dist), t(vis_in), tol, h, want_surface=True)
        assert np.array_equal(got.cpu().numpy(), want), h
        assert np.array_equal(surface.cpu().numpy(), want_surface, equal_nan=True), h
        assert (want != vis_in).any() and np.isnan(want_surface).any()
        assert np.isinf(want_surface).any() == (h <= 2)            # windows of background only, until the window holds the whole map
    for h in (9, -1):
        with pytest.raises(_lib.SmilError):
            engine.depth_visibility(t(depth), t(norm), t(dist), t(vis_in), tol, h)
    with pytest.raises(_lib.SmilError):                              # float32 keypoints are not taken: the comparison is float64
        engine.depth_visibility(t(depth), t(norm.astype(np.float32)), t(dist), t(vis_in), tol, 1)


def test_renderer_keypoint_visibility():
    """The sphere scene (2 frames x 3 views at S = 33): every point's visibility is the float64 restatement's; nothing is left out
    (tests/test_visibility_cpu.py::test_model_scene_margins)."""
    from smilify_amd.p3d_renderer import Renderer

    s = FR.visibility_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    r = Renderer(s.S, DEV, views=s.views)
    r.set_camera_parameters(t(s.R), t(s.T), t(s.fov))
    verts, faces, points = t(s.verts), t(s.faces)[None].expand(s.frames, -1, -1), t(s.points)
    got = r.keypoint_visibility(verts, points, faces, FR.VIS_TOLERANCE, FR.VIS_NEIGHBORHOOD, visibility=t(s.vis_in))
    assert got.shape == (s.N, s.points.shape[1]) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), s.expected), (got.cpu().numpy(), s.expected)
    # without a visibility coming in every point starts visible
    ones = r.keypoint_visibility(verts, points, faces, FR.VIS_TOLERANCE, FR.VIS_NEIGHBORHOOD).cpu().numpy()
    keep = s.vis_in != 0
    assert np.array_equal(ones[keep], s.expected[keep])
    # the distance map behind it, against float64 where the face is sure (a figure: its bound is test_fragments_on_edge_scenes')
    dist = r.render_depth(verts, faces, kind="distance").cpu().numpy()
    ok = np.isfinite(s.dist_map) & np.isfinite(dist) & ~s.unsure
    err = float(np.abs(dist[ok] - s.dist_map[ok]).max())
    print(f"model scene: {int(s.expected.size)} keypoints, {int((s.expected != s.vis_in).sum())} hidden; distance map error {err:.3e} on {int(ok.sum())} pixels")


def test_fitter_joint_self_occlusion(tables):
    """STICK, 2 frames x 2 views at S = 32: the fitter's answer is ``Renderer.keypoint_visibility`` of its own posed mesh and canonical
    joints, and calling it changes nothing a fit step sees."""
    from smilify_amd import synthetic

    weights, w_temp = synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL
    make = lambda: synthetic.make_problem(tables("stick"), 2, 2, 32, DEV, seed=11, window=2)  # noqa: E731
    fitter, plain = make(), make()
    losses = {id(fitter): [], id(plain): []}
    for f in (fitter, plain):
        f.begin_stage(synthetic.STAGE1_LR)
        losses[id(f)].append(f.fit_step(weights, w_temp, window=2).clone())
    target_vis = fitter.target_visibility.clone()
    vis = fitter.joint_self_occlusion(0.05)
    Jc = len(fitter.config.CANONICAL_MODEL_JOINTS)
    assert vis.shape == (2 * 2, Jc) and vis.dtype == torch.float32 and set(vis.unique().tolist()) <= {0.0, 1.0}
    verts, canon = fitter.posed_mesh()
    faces = fitter.smal_model.faces[None].expand(2, -1, -1)
    assert torch.equal(vis, fitter.renderer.keypoint_visibility(verts, canon, faces, 0.05, 1))
    assert torch.equal(fitter.target_visibility, target_vis)
    for f in (fitter, plain):
        losses[id(f)].append(f.fit_step(weights, w_temp, window=2).clone())
    torch.cuda.synchronize()
    # two fitters of one seed agree to the last bits of the gradients' float atomics: the tolerance tests/test_gpu_fitter_state.py
    # compares two fitters with.  A fit step that saw other cameras, targets or a stale cache would differ in the first digits.
    for a, b in zip(losses[id(fitter)], losses[id(plain)]):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-4, atol=1e-6)
    print(f"joint self-occlusion: {int((vis == 0).sum())} of {vis.numel()} joints hidden at tolerance 0.05")
