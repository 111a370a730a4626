"""The PointNet++ operations without a GPU: the restatements (tests/pointnet2_ref.py) against the reference's own run
(tests/golden/pointnet2_ref.npz, written by tests/golden/make_pointnet2_fixture.py), the conditions the fixture's clouds must meet for
a float32 evaluation to be comparable, and the library's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pointnet2_ref as R
from conftest import REPO


def test_fps_restatement_reproduces_the_reference_and_no_step_is_fragile():
    fx = R.fixture()
    start = fx["fps_idx"][:, 0]
    i64, gap = R.fps(fx["xyz"], 256, start, np.float64)
    i32, _ = R.fps(fx["xyz"], 256, start, np.float32)
    print(f"[pointnet2] fps: smallest relative gap between the two largest running distances {gap:.3g}")
    assert gap >= R.FPS_GAP, f"the fixture's clouds hold a fragile FPS step (gap {gap:.3g}): the input is at fault"
    assert np.array_equal(i64, fx["fps_idx"]) and np.array_equal(i32, fx["fps_idx"])
    assert np.array_equal(R.fps(fx["xyz"], 64, fx["sg_fps_idx"][:, 0])[0], fx["sg_fps_idx"])


@pytest.mark.parametrize("i", range(3))
def test_ball_restatement_reproduces_the_reference(i):
    fx = R.fixture()
    radius, nsample = R.FIXTURE_BALLS[i]
    for b in range(3):
        q = fx["xyz"][b][fx["fps_idx"][b]]
        amb = R.ball_ambiguous(fx["xyz"][b], q, radius, nsample)
        print(f"[pointnet2] ball r={radius} cloud {b}: {int(amb.sum())} of {len(amb)} rows ambiguous")
        assert amb.mean() <= 0.02, f"more than 2 % of the rows are ambiguous at r={radius}: the input is at fault"
        for dtype in (np.float32, np.float64):
            got = R.ball_query(fx["xyz"][b], q, radius, nsample, dtype)
            assert np.array_equal(got[~amb], fx[f"ball{i}_idx"][b][~amb])


def test_grouping_restatement_reproduces_the_reference():
    fx = R.fixture()
    for b in range(3):
        xyz, ft = fx["xyz"][b], fx["feats"][b]
        centres = xyz[fx["sg_fps_idx"][b]]
        assert np.array_equal(centres, fx["sg_new_xyz"][b])
        amb = R.ball_ambiguous(xyz, centres, 0.2, 32)
        idx = R.ball_query(xyz, centres, 0.2, 32, np.float32)
        g = R.group(xyz, centres, ft, idx).transpose(2, 1, 0)  # (S, K, C)
        assert amb.mean() <= 0.02
        assert np.array_equal(g[~amb], fx["sg_new_points"][b][~amb])
        assert np.array_equal(R.group(xyz, None, None, idx).transpose(2, 1, 0)[~amb], fx["sg_grouped_xyz"][b][~amb])
    z = R.group(xyz, centres, ft, np.full((64, 2), 1500))
    assert z.shape == (7, 2, 64) and not z.any()


@pytest.mark.parametrize("key", ["msg", "sa", "sa_all"])
def test_layer_restatement_reproduces_the_reference(key):
    """The torch restatement in float64, on the restated indices, against the reference's float32 outputs and gradients: within a few
    float32 roundings of the largest value (centres whose ball rows are ambiguous are left out)."""
    fx = R.fixture()
    sd = R.state_dict(fx, key + "_sd.")
    xyz = torch.from_numpy(fx["xyz"]).double()
    ft = torch.from_numpy(fx["feats"]).double().requires_grad_(True)
    clear = np.ones((3, fx[key + "_out"].shape[2]), bool)
    if key == "sa_all":
        new_xyz, out = R.torch_sa(xyz, ft, sd, None, None, 2)
    else:
        torch.manual_seed(int(fx[key + "_seed"]))  # the reference's first draw under the seed: the start indices
        start = torch.randint(0, 1500, (3,), dtype=torch.long).numpy()
        fps_idx, _ = R.fps(fx["xyz"], 64, start)
        balls = list(zip([0.1, 0.2, 0.4], [8, 16, 32])) if key == "msg" else [(0.3, 16)]
        idx = []
        for r, k in balls:
            rows = [R.ball_query(fx["xyz"][b], fx["xyz"][b][fps_idx[b]], r, k) for b in range(3)]
            idx.append(torch.from_numpy(np.stack(rows)))
            clear &= ~np.stack([R.ball_ambiguous(fx["xyz"][b], fx["xyz"][b][fps_idx[b]], r, k) for b in range(3)])
        f = torch.from_numpy(fps_idx)
        new_xyz, out = R.torch_msg(xyz, ft, sd, f, idx, [2, 2, 2]) if key == "msg" else R.torch_sa(xyz, ft, sd, f, idx[0], 2)
    assert np.array_equal(new_xyz.float().numpy(), fx[key + "_new_xyz"])
    assert clear.mean() >= 0.9
    err = np.abs(out.detach().numpy() - fx[key + "_out"]).transpose(0, 2, 1)[clear]
    print(f"[pointnet2] {key}: output max abs err {err.max():.3g} (max |value| {np.abs(fx[key + '_out']).max():.3g})")
    assert err.max() <= 64 * R.U * np.abs(fx[key + "_out"]).max()
    if clear.all():
        (out * torch.from_numpy(fx[key + "_probe"]).double()).sum().backward()
        e = np.abs(ft.grad.numpy() - fx[key + "_d_feats"]).max()
        assert e <= 256 * R.U * np.abs(fx[key + "_d_feats"]).max(), e


def test_ambiguity_marks_on_a_grid():
    """A candidate exactly on the sphere is inside and marks its row ambiguous; one well inside or outside does not."""
    xyz = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.25, 0, 0], [2.0, 0, 0]])
    q = np.array([[0.0, 0, 0], [5.0, 5, 5]])
    assert R.ball_query(xyz, q, 0.5, 8).tolist() == [[0, 1, 2, 0], [4, 4, 4, 4]]
    assert R.ball_ambiguous(xyz, q, 0.5, 8).tolist() == [True, False]
    assert R.ball_ambiguous(xyz, q, 0.4, 8).tolist() == [False, False]
    assert R.ball_ambiguous(xyz, q, 0.5, 1).tolist() == [False, False]  # full at index 0: the candidate on the sphere is never looked at
    idx, gap = R.fps(np.array([[[0.0, 0, 0], [1, 0, 0], [1, 0, 0], [0.5, 0, 0]]]), 5, [0])
    assert idx.tolist() == [[0, 1, 3, 0, 0]] and gap == 0.0  # the tie of points 1 and 2 goes to the smaller index


def test_argument_validation_without_gpu():
    from smilify_amd import _lib

    lib = _lib.load()
    assert _lib.FPS_MAX_N == 16384
    header = open(os.path.join(REPO, "include", "smilfit.h")).read()
    assert "#define SMIL_FPS_MAX_N 16384" in header and "#define SMIL_BALL_MAX_RADII 4" in header

    def err():
        return lib.smil_last_error()

    assert lib.smil_fps(None, None, 1, 0, 4, None, None) == -1 and b"N=0" in err()
    assert lib.smil_fps(None, None, 1, 8, 0, None, None) == -1 and b"npoint=0" in err()
    assert lib.smil_fps(None, None, 1, _lib.FPS_MAX_N + 1, 4, None, None) == -3 and b"SMIL_FPS_MAX_N" in err()
    assert lib.smil_fps(None, None, 1, _lib.FPS_MAX_N, 4, None, None) == -1 and b"null" in err()
    r, k, o = (ctypes.c_double * 5)(*[0.1] * 5), (ctypes.c_int32 * 5)(*[4] * 5), (ctypes.c_void_p * 5)()
    assert lib.smil_ball_query(None, None, 1, 8, 4, 5, r, k, o, None) == -1 and b"n_radii=5" in err()
    assert lib.smil_ball_query(None, None, 1, 8, 4, 0, r, k, o, None) == -1 and b"n_radii=0" in err()
    assert lib.smil_ball_query(None, None, 1, 0, 4, 1, r, k, o, None) == -1 and b"N=0" in err()
    k[1] = 0
    assert lib.smil_ball_query(None, None, 1, 8, 4, 2, r, k, o, None) == -1 and b"nsample[1]=0" in err()
    assert lib.smil_ball_query(None, None, 1, 8, 4, 1, r, k, o, None) == -1 and b"null" in err()
    assert lib.smil_group_points(None, None, None, None, 1, 0, 4, 2, 3, 0, None, None) == -1 and b"N=0" in err()
    assert lib.smil_group_points(None, None, None, None, 1, 8, 4, 2, 3, 0, None, None) == -1 and b"null" in err()
    assert lib.smil_group_points_backward(None, None, 1, 8, 4, 2, 0, 1, 0, None, None, None) == -1 and b"D=0" in err()
    assert lib.smil_group_points_backward(None, None, 1, 8, 4, 2, 3, 1, 0, None, None, None) == -1 and b"null" in err()
    assert lib.smil_group_points_backward_workspace_bytes(2, 5, 0) == 0 and lib.smil_group_points_backward_workspace_bytes(2, 5, 3) > 0


def test_python_checks_without_gpu():
    from smilify_amd import _lib, engine, pointnet2

    pc = pointnet2.pc_normalize(np.array([[0.0, 0, 0], [2, 0, 0], [0, 4, 0]]))
    assert np.allclose(pc.mean(0), 0) and np.isclose(np.sqrt((pc ** 2).sum(1)).max(), 1.0)
    a, b = torch.rand(2, 5, 3), torch.rand(2, 7, 3)
    assert torch.allclose(pointnet2.square_distance(a, b), torch.cdist(a, b) ** 2, atol=1e-5)
    new_xyz, pts = pointnet2.sample_and_group_all(a, torch.rand(2, 5, 4))
    assert new_xyz.shape == (2, 1, 3) and not new_xyz.any() and pts.shape == (2, 1, 5, 7)
    with pytest.raises(ValueError, match="SMIL_FPS_MAX_N"):
        engine.fps(torch.zeros(1, _lib.FPS_MAX_N + 1, 3), 4, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        engine.ball_query(a, a, [0.1] * 5, [4] * 5)
    with pytest.raises(ValueError):
        engine.ball_query(a, a, [0.1], [0])
    with pytest.raises(ValueError):
        pointnet2.farthest_point_sample(a, 3, start_idx=torch.tensor([0, 5]))
    with pytest.raises(_lib.SmilError):
        pointnet2.farthest_point_sample(a, 3)  # no CPU path
    sa = pointnet2.PointNetSetAbstractionMsg(8, [0.1, 0.2], [4, 8], 5, [[8, 8], [8, 16]])
    assert [k for k in sa.state_dict() if "num_batches" not in k][:2] == ["conv_blocks.0.0.weight", "conv_blocks.0.0.bias"]
    assert sa.conv_blocks[1][0].in_channels == 8
