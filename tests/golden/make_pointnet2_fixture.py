"""Writes tests/golden/pointnet2_ref.npz: the reference's own fitter_3d/pointcloud2smil/pointnet2_utils.py on the CPU, in float32 as
the reference runs it.

    python tests/golden/make_pointnet2_fixture.py /path/to/reference/checkout

Three clouds of 1 500 vertices of the Atta scan (tests/golden/atta_worker_mesh.npz), each a seeded draw without replacement,
``pc_normalize``d.  Recorded: farthest_point_sample to 256 under a seed; query_ball_point of those centres at (0.1, 16), (0.2, 32) and
(0.4, 128); sample_and_group(returnfps=True) with 4 feature channels; one PointNetSetAbstractionMsg and two PointNetSetAbstraction
(group_all False and True) in eval() with seeded weights and batch-norm statistics: inputs, outputs, the state_dict and the gradients
of sum(output * probe) to the weights and to the input features.  The file holds data only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, D = 1500, 4
SEED_CLOUDS, SEED_FPS, SEED_SG, SEED_MSG, SEED_SA = 11, 12, 13, 14, 15
BALLS = ((0.1, 16), (0.2, 32), (0.4, 128))
MSG = dict(npoint=64, radius_list=[0.1, 0.2, 0.4], nsample_list=[8, 16, 32], in_channel=D, mlp_list=[[8, 8], [8, 12], [8, 16]])
SA = dict(npoint=64, radius=0.3, nsample=16, in_channel=3 + D, mlp=[8, 16], group_all=False)
SA_ALL = dict(npoint=None, radius=None, nsample=None, in_channel=3 + D, mlp=[8, 16], group_all=True)


def seeded(module, seed):
    """Seeded weights, and batch-norm statistics and affine terms away from their defaults, in eval()."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            r = torch.randn(t.shape, generator=g)
            positive = name.endswith("running_var") or (name.endswith(".weight") and t.dim() == 1)  # variances and batch-norm scales
            t.copy_(0.5 + r.abs() if positive else 0.5 * r)
    return module.eval()


def run_module(module, xyz, feats, seed, out, key):
    torch.manual_seed(seed)
    f = feats.clone().requires_grad_(True)
    new_xyz, new_points = module(xyz.permute(0, 2, 1), f.permute(0, 2, 1))
    probe = torch.randn(new_points.shape, generator=torch.Generator().manual_seed(seed + 100))
    (new_points * probe).sum().backward()
    out[key + "_seed"] = np.int64(seed)
    out[key + "_new_xyz"], out[key + "_out"], out[key + "_probe"] = new_xyz.detach().numpy(), new_points.detach().numpy(), probe.numpy()
    out[key + "_d_feats"] = f.grad.numpy()
    for name, t in module.state_dict().items():
        out[f"{key}_sd.{name}"] = t.detach().numpy()
    for name, p in module.named_parameters():
        out[f"{key}_grad.{name}"] = p.grad.numpy()


def main():
    spec = importlib.util.spec_from_file_location(
        "pointnet2_utils", os.path.join(sys.argv[1], "fitter_3d", "pointcloud2smil", "pointnet2_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    verts = np.load(os.path.join(HERE, "atta_worker_mesh.npz"))["verts"]
    rng = np.random.default_rng(SEED_CLOUDS)
    clouds = np.stack([ref.pc_normalize(verts[rng.permutation(len(verts))[:N]]) for _ in range(3)]).astype(np.float32)
    feats = rng.standard_normal((3, N, D)).astype(np.float32)
    xyz, ft = torch.from_numpy(clouds), torch.from_numpy(feats)
    out = dict(xyz=clouds, feats=feats)

    torch.manual_seed(SEED_FPS)
    fps_idx = ref.farthest_point_sample(xyz, 256)
    out["fps_seed"], out["fps_idx"] = np.int64(SEED_FPS), fps_idx.numpy().astype(np.int16)
    new_xyz = ref.index_points(xyz, fps_idx)
    for i, (r, k) in enumerate(BALLS):
        out[f"ball{i}_idx"] = ref.query_ball_point(r, k, xyz, new_xyz).numpy().astype(np.int16)

    torch.manual_seed(SEED_SG)
    sg = ref.sample_and_group(64, 0.2, 32, xyz, ft, returnfps=True)
    out["sg_seed"] = np.int64(SEED_SG)
    out["sg_new_xyz"], out["sg_new_points"], out["sg_grouped_xyz"] = (t.numpy() for t in sg[:3])
    out["sg_fps_idx"] = sg[3].numpy().astype(np.int16)

    run_module(seeded(ref.PointNetSetAbstractionMsg(**MSG), SEED_MSG), xyz, ft, SEED_MSG, out, "msg")
    run_module(seeded(ref.PointNetSetAbstraction(**SA), SEED_SA), xyz, ft, SEED_SA, out, "sa")
    run_module(seeded(ref.PointNetSetAbstraction(**SA_ALL), SEED_SA + 1), xyz, ft, SEED_SA + 1, out, "sa_all")

    path = os.path.join(HERE, "pointnet2_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
