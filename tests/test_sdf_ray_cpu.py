"""The spatial-diameter ray cast without a GPU: the float64 restatement (tests/sdf_ray_ref.py) against the reference's own run
(tests/golden/sdf_ray_ref.npz, written by tests/golden/make_sdf_ray_fixture.py), the share of rays a float32 evaluation may decide
differently on the meshes the GPU tests use, and the file formats of smilify_amd.sdf."""
import os
import pickle

import numpy as np
import pytest
import torch

import sdf_ray_ref as R

U = R.U


@pytest.mark.parametrize("name", ["all", "sampled"])
def test_restatement_reproduces_the_reference(name):
    g, o, c, diam = R.fixture_case(name)
    v, f = g["verts"], g["faces"]
    S = len(o)
    assert g[name + "_dirs"].shape == (S, int(g["num_rays"]), 3) and S == (len(f) if name == "all" else 12)
    if name == "all":
        assert np.array_equal(g["all_face_idx"], np.arange(len(f)))
        assert np.abs(g["all_points"] - v[f].mean(1)).max() <= 4 * U * np.abs(v).max()
    else:  # the cap of 6 valid rays bites: the fixture would not notice a walk that ignored it otherwise
        _, d_lo, d_hi, _ = R.thresholds(v)
        assert (((c["t"] > d_lo) & (c["t"] < d_hi)).sum(1) > S // 2).any()
    clear = ~c["ambiguous"].any(1)
    rel = np.abs(diam - g[name + "_diam"]) / np.abs(diam)
    print(f"[sdf-ray] {name}: {int((~clear).sum())} of {S} samples hold an ambiguous ray; diameters of the others: max rel err "
          f"{rel[clear].max() / U:.2f} x 2^-24")
    assert clear.sum() >= 0.9 * S
    assert (rel[clear] <= 8 * U).all()
    k_smooth, k_vertex = (int(k) for k in g[name + "_k"])
    sm, det = R.smooth(g[name + "_points"], g[name + "_diam"], k_smooth)
    rs = np.abs(sm - g[name + "_smoothed"]) / np.abs(sm)
    print(f"[sdf-ray] {name}: smoothed max rel err {rs[det].max() / U:.2f} x 2^-24 on {int(det.sum())} of {S} determined rows")
    assert det.sum() >= 0.9 * S and (rs[det] <= 8 * U).all()
    vs, detv, _ = R.vertex_values(v, g[name + "_points"], g[name + "_smoothed"], k_vertex)
    ev = np.abs(vs - g[name + "_vertex_sdf"])  # values scaled to [0, 1]: absolute
    print(f"[sdf-ray] {name}: vertex values max abs err {ev[detv].max():.3g} on {int(detv.sum())} of {len(v)} determined rows")
    assert detv.sum() >= 0.9 * len(v) and (ev[detv] <= 8 * U).all()
    assert vs.min() == 0.0 and vs.max() == 1.0


@pytest.mark.parametrize("name", ["fixture", "atta", "stick"])
def test_few_rays_are_ambiguous(name):
    """The condition of the GPU comparison: at most 1 % of the rays may be decided differently by a float32 evaluation, and at most
    10 % of the samples hold such a ray."""
    case = R.condition_case(name)
    amb = case["cast"]["ambiguous"]
    print(f"[sdf-ray] {name}: {int(amb.sum())} of {amb.size} rays ambiguous, {int(amb.any(1).sum())} of {len(amb)} samples hold one")
    assert amb.shape == (min(400, len(case["faces"])), 30)
    assert amb.sum() <= 0.01 * amb.size
    assert amb.any(1).sum() <= 0.10 * len(amb)


def test_classification_on_a_box():
    """A ray through an edge, a corner or the diagonal of a side of a box is ambiguous, a ray through the middle of a triangle is not;
    without the thresholds nothing is classified."""
    v, f = R.box(-1.0, 1.0)
    o = np.zeros((1, 3))
    d = np.array([[[1.0, 0.25, 0.5], [1.0, 1.0, 0.5], [1.0, 1.0, 1.0], [1.0, 0.5, -0.5 + 1e-5]]])  # middle of a side, its edges, a corner, its diagonal
    c = R.cast(v, f, o, [-1], d, 1e-3, 0.01, 10.0, 4.0)
    assert c["ambiguous"].tolist() == [[False, True, True, True]]
    assert np.allclose(c["t"], 1.0) and (c["face"] >= 0).all()
    assert not R.cast(v, f, o, [-1], d, 1e-3)["ambiguous"].any()
    assert R.diameters([[1.0, -1.0, 3.0, 2.0, 50.0]], 0.5, 10.0, 2).tolist() == [2.0]
    assert R.diameters([[-1.0, 0.25]], 0.5, 10.0, 2).tolist() == [0.5]


def test_file_formats_round_trip(tmp_path):
    from smilify_amd import fit3d, sdf

    r = dict(sample_points=torch.rand(5, 3), smoothed_diameters=torch.rand(5), vertex_sdf=torch.linspace(0, 1, 7), verts=torch.rand(7, 3),
             faces=torch.zeros(4, 3, dtype=torch.int64), num_samples=-1, num_rays=30, k_smoothing=50)
    path = sdf._save(r, str(tmp_path / "data"), "scan_01")
    assert os.path.basename(path) == "scan_01_sdf.pkl"
    with open(path, "rb") as fh:
        back = pickle.load(fh)
    assert set(back) == set(r) and all(not t.is_cuda for t in back.values() if isinstance(t, torch.Tensor))
    got = fit3d.load_sdf_values("scan_01.obj", str(tmp_path / "data"), "cpu")  # the .npz is preferred
    assert got.dtype == torch.float32 and torch.equal(got, r["vertex_sdf"])
    os.remove(tmp_path / "data" / "scan_01_sdf.npz")
    assert torch.equal(fit3d.load_sdf_values("scan_01", str(tmp_path / "data"), "cpu"), r["vertex_sdf"])
    args = sdf.build_parser().parse_args(["meshes", "--model", "m.npz"])
    assert (args.num_samples, args.num_rays, args.k_smoothing, args.seed, args.output_dir) == (-1, 30, 50, 0, "sdf_batch_output")
    for fn in (sdf.visualize_sdf, sdf.visualize_vertex_sdf, sdf.debug_single_vertex):
        with pytest.raises(NotImplementedError):
            fn()
    with pytest.raises(NotImplementedError):
        sdf.process_obj_file("x.obj", debug_mode=True)
