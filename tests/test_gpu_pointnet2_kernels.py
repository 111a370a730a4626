"""The PointNet++ kernels (csrc/pointnet2.hip) on the GPU against the restatements of tests/pointnet2_ref.py: exact index equality on
dyadic grids (coordinates are multiples of 1/8: float32 is exact, ties and candidates exactly on the sphere are many) and on the
reference's own run (tests/golden/pointnet2_ref.npz), bit equality of the grouped tensor with plain torch, and the grouping gradient
against float64."""
import numpy as np
import pytest
import torch

import pointnet2_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def grid(rng, *shape):
    return (rng.integers(-8, 9, shape + (3,)) / 8.0).astype(np.float32)


def gpu_fps(xyz, npoint, start):
    from smilify_amd import pointnet2

    out = pointnet2.farthest_point_sample(torch.from_numpy(xyz).to(DEV), npoint, start_idx=torch.from_numpy(np.asarray(start, np.int64)))
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(xyz), npoint)
    return out.cpu().numpy()


# N = 257, 513, 4097 change the points per thread (4 -> 8, one wave -> several, 4 -> 8 again); 1025 adds a wave
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 513, 1023, 1024, 1025, 4097])
def test_fps_on_a_dyadic_grid(N):
    rng = np.random.default_rng(N)
    xyz = grid(rng, 3, N)
    start = rng.integers(0, N, 3)
    ref, _ = R.fps(xyz, N + 3, start)
    assert (ref[:, N:] == 0).all()  # npoint > N: every distance is 0 in the end and index 0 wins
    for npoint in (1, N, N + 3):
        assert np.array_equal(gpu_fps(xyz, npoint, start), ref[:, :npoint]), npoint


@pytest.mark.parametrize("B,N", [(1, 65), (300, 257), (300, 700)])
def test_fps_batches(B, N):
    rng = np.random.default_rng(B + N)
    xyz = grid(rng, B, N)
    start = rng.integers(0, N, B)
    assert np.array_equal(gpu_fps(xyz, 40, start), R.fps(xyz, 40, start)[0])


def test_fps_reference_clouds_limit_and_determinism():
    from smilify_amd import _lib, pointnet2

    fx = R.fixture()
    got = gpu_fps(fx["xyz"], 256, fx["fps_idx"][:, 0])
    assert np.array_equal(got, fx["fps_idx"])
    assert np.array_equal(got, gpu_fps(fx["xyz"], 256, fx["fps_idx"][:, 0]))
    torch.manual_seed(int(fx["fps_seed"]))  # the start indices come from the default CPU generator, as the reference's on the CPU
    assert np.array_equal(pointnet2.farthest_point_sample(torch.from_numpy(fx["xyz"]).to(DEV), 256).cpu().numpy(), fx["fps_idx"])
    rng = np.random.default_rng(5)
    for N in (8193, _lib.FPS_MAX_N):
        big = rng.standard_normal((1, N, 3)).astype(np.float32)
        assert np.array_equal(gpu_fps(big, 48, [N - 1]), R.fps(big, 48, [N - 1], np.float32)[0])
    with pytest.raises(ValueError, match="SMIL_FPS_MAX_N"):
        gpu_fps(np.zeros((1, _lib.FPS_MAX_N + 1, 3), np.float32), 4, [0])


RADII = [0.25, 0.5, 0.75, 1.25]  # r^2 = 4/64, 16/64, 36/64, 100/64: grid points lie exactly on every sphere


@pytest.mark.parametrize("N", [63, 64, 65, 255, 256, 257])
def test_ball_query_on_a_dyadic_grid(N):
    from smilify_amd import engine, pointnet2

    rng = np.random.default_rng(N)
    xyz = grid(rng, N)
    xyz[N // 2] = (3.0, 3.0, 3.0)  # an isolated point: its query has one hit, padded
    q = np.concatenate([xyz[rng.integers(0, N, 60)], xyz[N // 2][None], np.full((1, 3), 5.0, np.float32), grid(rng, 8)])
    d2 = R.sqdist(xyz[None], q[:, None], np.float64)
    tx, tq = torch.from_numpy(xyz[None]).to(DEV), torch.from_numpy(q[None]).to(DEV)
    single = {}
    for radius in RADII:
        assert (d2 == radius * radius).sum() > 0
        for nsample in (1, 16, 128, N + 5):
            ref = R.ball_query(xyz, q, radius, nsample)
            got = pointnet2.query_ball_point(radius, nsample, tx, tq)
            assert got.dtype == torch.int64 and tuple(got.shape) == (1, len(q), min(nsample, N))
            assert np.array_equal(got[0].cpu().numpy(), ref), (radius, nsample)
            single[radius, nsample] = ref
    assert (single[0.25, 16][60] == N // 2).all() and (single[1.25, 16][61] == N).all()  # one hit padded; no hit: a row of N
    assert (single[1.25, 16][:60].max(1) < 64).any()  # a ball that is full inside the first 64 candidates
    ns = [16, 1, N + 5, 128]
    for n in (1, 2, 3, 4):
        outs = engine.ball_query(tx, tq, RADII[:n], ns[:n])
        assert len(outs) == n and all(o.dtype == torch.int32 for o in outs)
        for o, radius, k in zip(outs, RADII, ns):
            assert np.array_equal(o[0].cpu().numpy(), single[radius, k]), (n, radius, k)


def test_ball_query_reference_clouds():
    from smilify_amd import engine

    fx = R.fixture()
    xyz = torch.from_numpy(fx["xyz"]).to(DEV)
    centres = torch.from_numpy(np.stack([fx["xyz"][b][fx["fps_idx"][b]] for b in range(3)])).to(DEV)
    outs = engine.ball_query(xyz, centres, [r for r, _ in R.FIXTURE_BALLS], [k for _, k in R.FIXTURE_BALLS])
    again = engine.ball_query(xyz, centres, [r for r, _ in R.FIXTURE_BALLS], [k for _, k in R.FIXTURE_BALLS])
    for i, (radius, nsample) in enumerate(R.FIXTURE_BALLS):
        assert torch.equal(outs[i], again[i])
        for b in range(3):
            amb = R.ball_ambiguous(fx["xyz"][b], centres[b].cpu().numpy(), radius, nsample)
            assert amb.mean() <= 0.02
            assert np.array_equal(outs[i][b].cpu().numpy()[~amb], fx[f"ball{i}_idx"][b][~amb]), (radius, b)


@pytest.mark.parametrize("S,K", [(7, 9), (8, 8), (13, 5), (1, 1), (40, 11)])
@pytest.mark.parametrize("D", [0, 1, 3, 64, 320])
def test_grouping_forward_is_bit_equal_to_torch(S, K, D):
    from smilify_amd import engine

    B, N = 2, 50
    g = torch.Generator().manual_seed(S * 1000 + D)
    xyz = torch.randn(B, N, 3, generator=g).to(DEV)
    centres = torch.randn(B, S, 3, generator=g).to(DEV)
    feats = torch.randn(B, N, D, generator=g).to(DEV) if D else None
    idx = torch.randint(0, N, (B, S, K), generator=g).to(DEV)
    for xyz_last in (False, True):
        ref = R.torch_group(xyz, centres, feats, idx, xyz_last)
        got = engine.group_points(xyz, centres, feats, idx.int(), xyz_last)
        assert got.is_contiguous() and torch.equal(got, ref), xyz_last
    bad = idx.clone()
    bad[0, 0, 0], bad[1, S - 1, K - 1] = N, -1
    ref = R.torch_group(xyz, centres, feats, idx)
    ref[0, :, 0, 0] = 0
    ref[1, :, K - 1, S - 1] = 0
    assert torch.equal(engine.group_points(xyz, centres, feats, bad.int()), ref)
    if D:
        assert torch.equal(engine.group_points(None, None, feats, idx.int()), R.torch_group(None, None, feats, idx))
    assert torch.equal(engine.group_points(xyz, None, None, idx.int()), R.torch_group(xyz, None, None, idx))


def test_index_points_shapes():
    from smilify_amd import pointnet2

    g = torch.Generator().manual_seed(3)
    pts = torch.randn(2, 30, 5, generator=g).to(DEV)
    i2, i3 = torch.randint(0, 30, (2, 9), generator=g).to(DEV), torch.randint(0, 30, (2, 9, 4), generator=g).to(DEV)
    rows = torch.arange(2, device=DEV)
    assert torch.equal(pointnet2.index_points(pts, i2), pts[rows[:, None], i2])
    assert torch.equal(pointnet2.index_points(pts, i3), pts[rows[:, None, None], i3])


@pytest.mark.parametrize("D,xyz_last", [(5, False), (70, True)])
def test_grouping_backward_against_float64(D, xyz_last):
    from smilify_amd import pointnet2

    B, N, S, K = 2, 20, 16, 8
    g = torch.Generator().manual_seed(D)
    xyz, centres = torch.randn(B, N, 3, generator=g).to(DEV), torch.randn(B, S, 3, generator=g).to(DEV)
    idx = torch.randint(0, N - 1, (B, S, K), generator=g)  # point N - 1 is never drawn: its gradient is an exact zero
    idx[0, 3] = 7                                            # a row of K duplicates
    idx[1, 5, 2] = N                                         # outside: no gradient
    # magnitudes over 2^-6 .. 2^6: the sum is fixed point with a unit of 2^(7 + 8 - 61) here (largest |gradient| < 2^7, K S = 2^7
    # addends), so an addend is rounded by 2^-47 at most: inside 2^-24 |addend| for everything above 2^-23
    d_out = torch.randn(B, 3 + D, K, S, generator=g) * torch.exp2(torch.randint(-6, 7, (B, 3 + D, K, S), generator=g).float())
    off = 0 if xyz_last else 3
    d_out[:, off + 2] = 0.0                                  # a feature channel without gradient
    grads = []
    for _ in range(2):
        feats = torch.randn(B, N, D, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
        pointnet2._group(xyz, centres, feats, idx.to(DEV), xyz_last).backward(d_out.to(DEV))
        grads.append(feats.grad.cpu())
    assert torch.equal(grads[0], grads[1])
    ref, mag = np.zeros((B, N + 1, D)), np.zeros((B, N + 1, D))
    add = d_out[:, off:off + D].double().numpy().transpose(0, 3, 2, 1)  # (B, S, K, D)
    for b in range(B):
        np.add.at(ref[b], idx[b].numpy(), add[b])
        np.add.at(mag[b], idx[b].numpy(), np.abs(add[b]))
    err = np.abs(grads[0].double().numpy() - ref[:, :N])
    print(f"[pointnet2] grouping backward D={D}: max err / (2^-24 sum|addends|) = {(err / np.maximum(mag[:, :N], 1e-300)).max() / R.U:.3g}")
    assert (err <= 8 * R.U * mag[:, :N]).all()
    assert not grads[0][:, N - 1].any() and not grads[0][:, :, 2].any() and grads[0].abs().sum() > 0
    with pytest.raises(NotImplementedError):
        pointnet2._group(xyz.clone().requires_grad_(True), centres, feats, idx.to(DEV))
    with pytest.raises(NotImplementedError):
        pointnet2.sample_and_group(4, 0.5, 4, xyz.clone().requires_grad_(True), None)


def test_grouping_backward_scales_exactly_with_the_gradient():
    """The fixed-point unit follows the cloud's largest |gradient|: d_out times 2^k gives feats.grad times 2^k, bit for bit, and an
    all-zero d_out (a recorded maximum of 0) exact zeros."""
    from smilify_amd import pointnet2

    B, N, S, K, D = 2, 20, 16, 8, 5
    g = torch.Generator().manual_seed(D)
    xyz, centres = torch.randn(B, N, 3, generator=g).to(DEV), torch.randn(B, S, 3, generator=g).to(DEV)
    idx = torch.randint(0, N - 1, (B, S, K), generator=g)
    idx[0, 3] = 7  # a row of K duplicates
    d_out = torch.randn(B, 3 + D, K, S, generator=g) * torch.exp2(torch.randint(-6, 7, (B, 3 + D, K, S), generator=g).float())

    def grad(d):
        feats = torch.randn(B, N, D, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
        pointnet2._group(xyz, centres, feats, idx.to(DEV), False).backward(d.to(DEV))
        return feats.grad.cpu()

    base = grad(d_out)
    assert base.abs().sum() > 0
    for k in (-40, 0, 40):
        assert torch.equal(grad(d_out * 2.0 ** k), base * 2.0 ** k), k
    zero = grad(torch.zeros_like(d_out))
    assert torch.equal(zero, torch.zeros_like(zero))
