"""CPU-side checks of the point <-> mesh distances: the library's new surface, and the restatement (tests/point_mesh_ref.py) that the
GPU tests compare the kernels with - against hand cases with known answers, against float64 autograd and against a second,
independent formulation."""
import os
import re

import numpy as np
import pytest
import torch

import point_mesh_cases as PC
import point_mesh_ref as PR
from conftest import REPO


def test_library_surface():
    from smilify_amd import _lib

    lib = _lib.load()
    for name in ("smil_point_mesh_workspace_bytes", "smil_point_face_distance", "smil_face_point_distance", "smil_point_mesh_backward"):
        assert hasattr(lib, name), name
    v = lib.smil_version()
    assert b"0.11" in v and b"point-mesh distances" in v, v
    small, large = lib.smil_point_mesh_workspace_bytes(2, 100, 50, 60), lib.smil_point_mesh_workspace_bytes(2, 1000, 500, 600)
    assert 0 < small < large and small % 256 == 0
    assert lib.smil_point_mesh_workspace_bytes(0, 100, 50, 60) == 0 and lib.smil_point_mesh_workspace_bytes(2, 0, 50, 60) == 0
    # bad arguments are refused before anything is launched
    assert lib.smil_point_face_distance(None, 1, None, None, 1, 1, 1, None, 1, None, 0, None, None, None, None, None) == -1
    assert b"null argument" in lib.smil_last_error()
    src = open(os.path.join(REPO, "smilify_amd", "csrc", "point_mesh.hip")).read()
    assert int(re.search(r"#define PM_TILE (\d+)", src).group(1)) == PC.TILE


def test_python_surface_without_gpu():
    from smilify_amd import fit3d, mesh3d

    for name in ("point_face_distance", "face_point_distance", "point_mesh_face_distance"):
        assert callable(getattr(fit3d, name))
    assert mesh3d.ClosestPoints._fields == ("dist2", "face", "bary", "points")
    assert "w_surface" not in fit3d.default_weights
    assert fit3d.build_parser().parse_args(["--mesh_dir", "x"]).w_surface == 0.0
    m = mesh3d.Meshes([torch.zeros(4, 3), torch.zeros(5, 3)], [torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.tensor([[2, 3, 4]])])
    t = m.face_tables()
    assert t.faces.dtype == torch.int32 and t.faces.tolist() == [[0, 1, 2], [1, 2, 3], [6, 7, 8]]
    assert t.face_off.tolist() == [0, 2, 3] and t.vert_off.tolist() == [0, 4, 9]
    assert (t.n_meshes, t.n_faces, t.max_faces, t.n_verts, t.max_verts) == (2, 3, 2, 9, 5)
    assert m.offset_verts(torch.zeros(9, 3)).face_tables() is t  # kept with the face arrays


@pytest.mark.parametrize("case", PC.HAND, ids=[c[0] for c in PC.HAND])
def test_restatement_hand_cases(case):
    _, tri, p, bary, d2 = case
    for dtype in (torch.float64, torch.float32):  # the 1/8 grid is exact in both
        got_b, got_d = PR.closest_on_triangle(torch.tensor(p, dtype=dtype), torch.tensor(tri, dtype=dtype))
        assert got_b.tolist() == [float(x) for x in bary], (dtype, got_b)
        assert float(got_d) == d2, (dtype, float(got_d))


@pytest.mark.parametrize("case", PC.DEGENERATE, ids=[c[0] for c in PC.DEGENERATE])
def test_restatement_degenerate_cases(case):
    _, tri, p, closest, d2 = case
    t = torch.tensor(tri, dtype=torch.float64)
    bary, got = PR.closest_on_triangle(torch.tensor(p, dtype=torch.float64), t)
    assert torch.isfinite(bary).all() and (bary >= 0).all() and float(bary.sum()) == 1.0
    assert ((bary[:, None] * t).sum(0)).tolist() == [float(x) for x in closest]
    assert float(got) == d2


def test_restatement_regions_all_occur_on_a_seeded_soup():
    verts, faces = PC.random_mesh(1, 30, 200)
    pts = torch.from_numpy(PC.random_cloud(2, 300)).double()
    tri = torch.from_numpy(verts).double()[torch.from_numpy(faces)]
    bary, _ = PR.closest_on_triangle(pts[:, None], tri[None])
    kinds = {tuple(k) for k in (bary > 0).reshape(-1, 3).tolist()}
    assert len(kinds) == 7, kinds
    assert (bary >= 0).all() and ((bary.sum(-1) - 1).abs() <= 4e-16).all()


def test_restatement_gradient_against_autograd():
    verts, faces = PC.random_mesh(4, 25, 60, degenerate=True)
    pts = PC.random_cloud(5, 120)
    _, face = PR.point_face(verts, faces, pts)
    g = torch.from_numpy(np.random.default_rng(6).standard_normal(len(pts)))
    v = torch.from_numpy(verts).double().requires_grad_(True)
    p = torch.from_numpy(pts).double().requires_grad_(True)
    _, d2 = PR.dist2_at(v, faces, p, face)
    want_p, want_v = torch.autograd.grad((g * d2).sum(), (p, v))
    got_p, got_v = PR.gradients_at(verts, faces, pts, face, g)
    assert torch.isfinite(want_p).all() and torch.isfinite(want_v).all()
    assert (got_p - want_p).abs().max() <= 1e-12 * want_p.abs().max()
    assert (got_v - want_v).abs().max() <= 1e-12 * want_v.abs().max()
    # ... and the other direction's records: several faces may pick one point
    _, point = PR.face_point(verts, faces, pts)
    gf = torch.from_numpy(np.random.default_rng(7).standard_normal(len(faces)))
    _, d2 = PR.dist2_at(v, faces, p, torch.arange(len(faces)), point)
    want_p, want_v = torch.autograd.grad((gf * d2).sum(), (p, v))
    got_p, got_v = PR.gradients_at(verts, faces, pts, torch.arange(len(faces)), gf, point)
    assert (got_p - want_p).abs().max() <= 1e-12 * want_p.abs().max()
    assert (got_v - want_v).abs().max() <= 1e-12 * want_v.abs().max()


@pytest.mark.parametrize("seed,scale", [(8, 1.0), (9, 2.0 ** -20), (10, 2.0 ** 12)])
def test_restatement_against_the_independent_formulation(seed, scale):
    """The region walk against the plane-or-segments form on a seeded soup, degenerate faces included: 1e-12 relative (of the squared
    distance, with the pair's squared extent as the floor for points on a face)."""
    verts, faces = PC.random_mesh(seed, 40, 300, scale=scale, degenerate=True)
    pts = torch.from_numpy(PC.random_cloud(seed + 100, 200, 1.5 * scale)).double()
    tri = torch.from_numpy(verts).double()[torch.from_numpy(faces)]
    on = (torch.rand(50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) + 0.05)
    on = ((on / on.sum(-1, keepdim=True))[..., None] * tri[:50]).sum(-2)  # points on faces
    pts = torch.cat([pts, on])
    _, d = PR.closest_on_triangle(pts[:, None], tri[None])
    want = PR.dist2_independent(pts[:, None], tri[None])
    extent = ((pts[:, None, None, :] - tri[None]) ** 2).sum(-1).max(-1).values
    err = ((d - want).abs() / (want + 1e-4 * extent + 1e-300)).max()  # (a point ON a face that is a point: 0 / 1e-300)
    assert float(err) <= 1e-12, float(err)
    assert float(PR.all_pairs(verts, faces, pts).min()) >= 0.0


def test_brute_force_and_loss_conventions():
    verts, faces = PC.random_mesh(12, 20, 33)
    pts = PC.random_cloud(13, 17)
    d = PR.all_pairs(verts, faces, pts)
    dp, fi = PR.point_face(verts, faces, pts)
    df, pi = PR.face_point(verts, faces, pts)
    assert torch.equal(dp, d.min(1).values) and torch.equal(df, d.min(0).values)
    assert torch.equal(d[torch.arange(17), fi], dp) and torch.equal(d[pi, torch.arange(33)], df)
    want = 0.5 * ((float(dp.mean()) + float(df.mean())) + (float(dp[:5].mean()) + float(PR.face_point(verts, faces, pts[:5])[0].mean())))
    assert abs(PR.loss([(verts, faces)] * 2, [pts, pts[:5]]) - want) <= 1e-15 * want
    # a non-finite point and a face with a non-finite vertex: inf and -1, never NaN; an empty cloud: -1 for every face
    bad_v = verts.copy()
    bad_v[faces[3, 1]] = np.nan
    bad_p = pts.copy()
    bad_p[2, 0] = np.inf
    d = PR.all_pairs(bad_v, faces, bad_p)
    assert not torch.isnan(d).any() and torch.isinf(d[2]).all() and torch.isinf(d[:, 3]).all()
    assert int(PR.point_face(bad_v, faces, bad_p)[1][2]) == -1
    assert (PR.face_point(verts, faces, pts[:0])[1] == -1).all()
    # the first of equal minima
    v, f, p, winner = PC.tie_fan()
    assert int(PR.point_face(v, f, p)[1][0]) == winner and float(PR.point_face(v, f, p)[0][0]) == 1.0
