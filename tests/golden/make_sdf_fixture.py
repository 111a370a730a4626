"""Writes tests/golden/sdf_distance_ref.npz: the reference's own SDF_distance (fitter_3d/utils.py) in float64 on small fixed inputs.

    python tests/golden/make_sdf_fixture.py /path/to/reference/checkout

The reference module is imported with ``pytorch3d`` and ``config`` stubbed (neither is needed by the function), and
``pytorch3d.ops.knn_points`` replaced by a brute-force torch search whose rows are ascending by (distance, index): a stable sort of
the squared distances.  Everything else - the z-scores, the softmax, the reductions, the two directions - is the reference's code.
The inputs are float32 numbers held as float64, so a float32 implementation is handed exactly what the reference was: the values
with the offset of 100 would otherwise move by 4e-6 in the cast, which is 1e-5 of their spread and shows in every softmax weight.
The file holds data only: the inputs, and per case the loss and both gradients.
"""
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

CASES = [  # name, k, batch_reduction, point_reduction, single_directional
    ("k50_mean_mean", 50, "mean", "mean", False),
    ("k50_sum_mean", 50, "sum", "mean", False),
    ("k50_mean_sum", 50, "mean", "sum", False),
    ("k50_sum_sum", 50, "sum", "sum", False),
    ("k50_single", 50, "mean", "mean", True),
    ("k1_mean_mean", 1, "mean", "mean", False),
    ("k1_single_sum_sum", 1, "sum", "sum", True),
]


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, **_):
    assert norm == 2
    d = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)
    order = torch.sort(d, dim=2, stable=True)[1][:, :, :K]
    return namedtuple("KNN", "dists idx knn")(torch.gather(d, 2, order), order, None)


def import_reference(root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    stub("pytorch3d")
    stub("pytorch3d.ops")
    stub("pytorch3d.ops.knn", knn_points=knn_points)
    stub("pytorch3d.io", load_obj=None)
    stub("pytorch3d.structures", Meshes=None)
    stub("config")
    sys.path.insert(0, root)
    import fitter_3d.utils as u

    return u


def main():
    u = import_reference(sys.argv[1])
    rng = np.random.RandomState(20)
    N, P1, P2 = 2, 70, 300
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    x = f32(rng.uniform(-1, 1, (N, P1, 3)))
    y = f32(rng.uniform(-1, 1, (N, P2, 3)))
    x_sdf = f32(rng.randn(N, P1) * 0.3 + 1.0)
    y_sdf = f32(100.0 + rng.randn(N, P2) * 0.3)  # a large common offset on one side
    out = dict(x=x, y=y, x_sdf=x_sdf, y_sdf=y_sdf, cases=np.array([c[0] for c in CASES]))
    for name, k, br, pr, single in CASES:
        X = torch.from_numpy(x).requires_grad_(True)
        Y = torch.from_numpy(y).requires_grad_(True)
        loss = u.SDF_distance(X, Y, torch.from_numpy(x_sdf), torch.from_numpy(y_sdf), k, batch_reduction=br, point_reduction=pr,
                              single_directional=single)
        gx, gy = torch.autograd.grad(loss, (X, Y))
        out[name + "_cfg"] = np.array([k, br == "sum", pr == "sum", single], np.int64)
        out[name + "_loss"] = np.float64(loss.item())
        out[name + "_dx"] = gx.numpy()
        out[name + "_dy"] = gy.numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sdf_distance_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
