"""The drop-in layers of smilify_amd.pointnet2 on the GPU against the reference's run (tests/golden/pointnet2_ref.npz).

The yardstick for outputs and gradients is the project's for float32 kernels: the result's largest error against a float64
evaluation on the CPU may be at most 4 x the largest error of the plain-torch float32 restatement (tests/pointnet2_ref.py) run on
the same GPU with the same weights and indices, plus a floor of 2^-24 max|value|."""
import numpy as np
import pytest
import torch

import pointnet2_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = {
    "msg": dict(npoint=64, radius_list=[0.1, 0.2, 0.4], nsample_list=[8, 16, 32], in_channel=4, mlp_list=[[8, 8], [8, 12], [8, 16]]),
    "sa": dict(npoint=64, radius=0.3, nsample=16, in_channel=7, mlp=[8, 16], group_all=False),
    "sa_all": dict(npoint=None, radius=None, nsample=None, in_channel=7, mlp=[8, 16], group_all=True),
}


def within(name, got, ref64, f32):
    e_got = (got.detach().double().cpu() - ref64).abs().max().item()
    e_f32 = (f32.detach().double().cpu() - ref64).abs().max().item()
    floor = R.U * ref64.abs().max().item()
    print(f"[pointnet2] {name}: error {e_got:.3g}, float32 torch restatement {e_f32:.3g}, floor {floor:.3g}")
    assert e_got <= 4 * e_f32 + floor, name


def build(key):
    from smilify_amd import pointnet2

    fx = R.fixture()
    cls = pointnet2.PointNetSetAbstractionMsg if key == "msg" else pointnet2.PointNetSetAbstraction
    layer = cls(**LAYERS[key])
    layer.load_state_dict(R.state_dict(fx, key + "_sd."), strict=True)
    return fx, layer.to(DEV).eval()


@pytest.mark.parametrize("key", ["msg", "sa", "sa_all"])
def test_layer_against_float64(key):
    from smilify_amd import pointnet2

    fx, layer = build(key)
    sd = R.state_dict(fx, key + "_sd.")
    xyz = torch.from_numpy(fx["xyz"]).to(DEV)
    feats = torch.from_numpy(fx["feats"]).to(DEV).requires_grad_(True)
    torch.manual_seed(int(fx[key + "_seed"]))
    new_xyz, out = layer(xyz.transpose(1, 2), feats.transpose(1, 2))
    assert np.array_equal(new_xyz.cpu().numpy(), fx[key + "_new_xyz"])  # the reference's centres: same start indices, same FPS
    probe = torch.from_numpy(fx[key + "_probe"])
    (out * probe.to(DEV)).sum().backward()
    grads = {n: p.grad for n, p in layer.named_parameters()}

    # the indices of the float64 evaluation: restated; a ball row that float32 may decide differently is taken from the product
    fps_idx, balls = None, []
    if key != "sa_all":
        torch.manual_seed(int(fx[key + "_seed"]))
        fps_idx, _ = R.fps(fx["xyz"], 64, torch.randint(0, 1500, (3,), dtype=torch.long).numpy())
        centres = np.stack([fx["xyz"][b][fps_idx[b]] for b in range(3)])
        pairs = list(zip(LAYERS[key]["radius_list"], LAYERS[key]["nsample_list"])) if key == "msg" else [(0.3, 16)]
        for r, k in pairs:
            ref = np.stack([R.ball_query(fx["xyz"][b], centres[b], r, k) for b in range(3)])
            amb = np.stack([R.ball_ambiguous(fx["xyz"][b], centres[b], r, k) for b in range(3)])
            got = pointnet2.query_ball_point(r, k, xyz, torch.from_numpy(centres).to(DEV)).cpu().numpy()
            assert amb.mean() <= 0.02 and np.array_equal(got[~amb], ref[~amb])
            balls.append(torch.from_numpy(np.where(amb[..., None], got, ref)))
        fps_idx = torch.from_numpy(fps_idx)

    def evaluate(dtype, dev):
        x = torch.from_numpy(fx["xyz"]).to(dev, dtype)
        f = torch.from_numpy(fx["feats"]).to(dev, dtype).requires_grad_(True)
        w = {n: (t.to(dev, dtype).requires_grad_(True) if t.is_floating_point() and "running" not in n else t.to(dev)) for n, t in sd.items()}
        fi = None if fps_idx is None else fps_idx.to(dev)
        if key == "msg":
            _, o = R.torch_msg(x, f, w, fi, [i.to(dev) for i in balls], [2, 2, 2])
        else:
            _, o = R.torch_sa(x, f, w, fi, balls[0].to(dev) if balls else None, 2)
        (o * probe.to(dev, dtype)).sum().backward()
        return o, f.grad, {n: t.grad for n, t in w.items() if t.requires_grad}

    o64, df64, g64 = evaluate(torch.float64, "cpu")
    o32, df32, g32 = evaluate(torch.float32, DEV)
    within(key + " output", out, o64, o32)
    within(key + " d features", feats.grad, df64, df32)
    assert set(grads) == set(g64)
    for n in sorted(grads):
        within(f"{key} d {n}", grads[n], g64[n], g32[n])


def test_sample_and_group_returns_the_reference_tensors():
    from smilify_amd import pointnet2

    fx = R.fixture()
    xyz, feats = torch.from_numpy(fx["xyz"]).to(DEV), torch.from_numpy(fx["feats"]).to(DEV)
    torch.manual_seed(int(fx["sg_seed"]))
    new_xyz, new_points, grouped_xyz, fps_idx = pointnet2.sample_and_group(64, 0.2, 32, xyz, feats, returnfps=True)
    assert (new_xyz.shape, new_points.shape, grouped_xyz.shape, fps_idx.shape) == ((3, 64, 3), (3, 64, 32, 7), (3, 64, 32, 3), (3, 64))
    assert (new_xyz.dtype, new_points.dtype, grouped_xyz.dtype, fps_idx.dtype) == (torch.float32,) * 3 + (torch.int64,)
    assert np.array_equal(fps_idx.cpu().numpy(), fx["sg_fps_idx"]) and np.array_equal(new_xyz.cpu().numpy(), fx["sg_new_xyz"])
    amb = np.stack([R.ball_ambiguous(fx["xyz"][b], fx["sg_new_xyz"][b], 0.2, 32) for b in range(3)])
    assert np.array_equal(new_points.cpu().numpy()[~amb], fx["sg_new_points"][~amb])
    assert np.array_equal(grouped_xyz.cpu().numpy()[~amb], fx["sg_grouped_xyz"][~amb])
    two = pointnet2.sample_and_group(64, 0.2, 32, xyz, None)
    assert len(two) == 2 and two[1].shape == (3, 64, 32, 3)


@pytest.mark.parametrize("S", [1, 2, 64])
def test_feature_propagation(S):
    from smilify_amd import pointnet2

    B, N, D1, D2 = 2, 150, 3, 5
    g = torch.Generator().manual_seed(S)
    xyz1, xyz2 = torch.randn(B, N, 3, generator=g), torch.randn(B, S, 3, generator=g)
    p1, p2 = torch.randn(B, N, D1, generator=g), torch.randn(B, S, D2, generator=g)
    layer = pointnet2.PointNetFeaturePropagation(D1 + D2, [8, 6]).eval()
    assert list(layer.state_dict())[:2] == ["mlp_convs.0.weight", "mlp_convs.0.bias"]
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    layer = layer.to(DEV)
    p2g = p2.to(DEV).requires_grad_(True)
    out = layer(xyz1.to(DEV).transpose(1, 2), xyz2.to(DEV).transpose(1, 2), p1.to(DEV).transpose(1, 2), p2g.transpose(1, 2))
    assert tuple(out.shape) == (B, 6, N)
    out.sum().backward()

    def evaluate(dtype, dev):
        q = p2.to(dev, dtype).requires_grad_(True)
        o = R.torch_fp(xyz1.to(dev, dtype), xyz2.to(dev, dtype), p1.to(dev, dtype), q, sd, 2)
        o.sum().backward()
        return o, q.grad

    o64, d64 = evaluate(torch.float64, "cpu")
    o32, d32 = evaluate(torch.float32, DEV)
    within(f"fp S={S} output", out, o64, o32)
    within(f"fp S={S} d points2", p2g.grad, d64, d32)
    bare = pointnet2.PointNetFeaturePropagation(D2, [4]).to(DEV).eval()  # without points1
    assert tuple(bare(xyz1.to(DEV).transpose(1, 2), xyz2.to(DEV).transpose(1, 2), None, p2.to(DEV).transpose(1, 2)).shape) == (B, 4, N)


def test_two_stacked_layers_train():
    from smilify_amd import pointnet2

    fx = R.fixture()
    torch.manual_seed(0)
    l1 = pointnet2.PointNetSetAbstractionMsg(48, [0.2, 0.4], [8, 16], 0, [[8, 8], [8, 16]]).to(DEV).train()
    l2 = pointnet2.PointNetSetAbstraction(12, 0.6, 8, 24 + 3, [16, 32], False).to(DEV).train()
    xyz = torch.from_numpy(fx["xyz"]).to(DEV).transpose(1, 2)
    x1, f1 = l1(xyz, None)
    x2, f2 = l2(x1, f1)
    assert tuple(x1.shape) == (3, 3, 48) and tuple(f1.shape) == (3, 24, 48) and tuple(x2.shape) == (3, 3, 12) and tuple(f2.shape) == (3, 32, 12)
    f2.square().sum().backward()
    params = list(l1.named_parameters()) + list(l2.named_parameters())
    assert len(params) == 24
    for n, p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert sum(float(p.grad.abs().sum()) for _, p in l1.named_parameters()) > 0  # the gradient crossed the second layer's grouping
