"""CPU checks of the colour (HardPhong) path: the C ABI declares, exports and binds it, the float64 restatement the GPU tests
judge it by (tests/shade_ref.py) gives hand-computed answers, and every scene of the edge tests (tests/colour_cases.py) reaches the
branch it was built for - shown from the restatement alone, so that a green GPU test cannot be one that missed its point."""
import os
import re

import numpy as np
import pytest
import torch

import colour_cases as cc
import shade_ref
from conftest import REPO
from oracle import render_ref

MESH_COLOR = np.array([0.0, 172.0, 223.0]) / 255.0


def test_colour_exports_are_declared_exported_and_bound():
    from smilify_amd import _lib

    header = open(os.path.join(REPO, "include", "smilfit.h")).read()
    for name in ("smil_colour_workspace_bytes", "smil_render_colour"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.smil_render_colour.argtypes is not None and len(lib.smil_render_colour.argtypes) == 9
    assert lib.smil_colour_workspace_bytes(None, 1, 64) == 0
    assert lib.smil_render_colour(None, None, None, None, None, None, None, None, None) == -1
    assert b"smil_render_colour" in lib.smil_last_error()


def _default_camera():
    R, T = render_ref.look_at_view_transform(2.7, 0.0, 0.0)  # the Renderer's camera: centre (0, 0, 2.7)
    return R, T


def test_known_answer_single_triangle_facing_the_camera():
    """A triangle in the plane z = 0 facing the default camera (and the light at (0, 0, 3)).  At S = 65 the centre pixel looks at
    the world origin: n = d = v = r = (0, 0, 1), so colour = (0.5 + 0.3) MESH_COLOR + 0.2.  A pixel outside is exactly 1."""
    S = 65
    verts = torch.tensor([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    faces = np.array([[0, 1, 2]])
    R, T = _default_camera()
    ndc = render_ref.project_to_ndc(verts[None], R, T, torch.tensor([60.0]))[0].numpy()
    img, p2f, unsure = shade_ref.render_colour(verts.numpy(), ndc, faces, R[0].numpy(), T[0].numpy(), MESH_COLOR, S)
    c = S // 2
    assert p2f[c, c] == 0 and not unsure[c, c]
    np.testing.assert_allclose(img[:, c, c], 0.8 * MESH_COLOR + 0.2, atol=1e-5)
    assert p2f[0, 0] == -1 and (img[:, 0, 0] == 1.0).all()
    # background everywhere the face is not
    assert (img[:, p2f < 0] == 1.0).all() and (p2f >= 0).sum() > 100


def test_pixel_centre_on_an_edge_is_background():
    """Strictly inside only: a pixel centre on an edge (a barycentric exactly 0) keeps no face; its neighbour inside does."""
    S = 16
    # output column xo has x_ndc = -1 + (2 (S - 1 - xo) + 1) / S; xo = 7 -> 1/16, so an edge at x = 1/16
    e = 1.0 / 16.0
    ndc = np.array([[e, -0.5, 1.0], [e, 0.5, 1.0], [e - 0.6, 0.0, 1.0]])
    faces = np.array([[0, 1, 2]])
    p2f, _, _, unsure = shade_ref.raster_k1(ndc, faces, S)
    row = 8  # y_ndc = -1 + (2 * 7 + 1) / 16 = -1/16, inside the face's y range
    assert p2f[row, 7] == -1 and unsure[row, 7]           # on the edge
    assert p2f[row, 8] == 0 and not unsure[row, 8]        # one pixel to the left of it in NDC: inside
    assert p2f[row, 6] == -1                               # the other side


def test_vertex_normals_of_a_closed_mesh():
    """Regular tetrahedron, faces outward: the (2 x area)-weighted corner normals of every vertex sum to its radial direction."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    n = shade_ref.vertex_normals(v, faces)
    np.testing.assert_allclose(n, v / np.sqrt(3.0), atol=1e-12)
    # area weighting: two coplanar faces of different size and one tilted face meeting at vertex 0
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-3, 0, 0], [0, 0, 1]], np.float64)
    f2 = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 1]])
    a = np.cross(v2[2] - v2[1], v2[0] - v2[1]) + np.cross(v2[3] - v2[2], v2[0] - v2[2]) + np.cross(v2[1] - v2[4], v2[0] - v2[4])
    np.testing.assert_allclose(shade_ref.vertex_normals(v2, f2)[0], a / np.linalg.norm(a), atol=1e-12)
    # a vertex of no face: zero (normalised with eps, not NaN)
    assert np.isfinite(shade_ref.vertex_normals(np.vstack([v, [[5, 5, 5]]]), faces)).all()


# ----------------------------------------------------------------------------------------------
# what the edge tests added to the restatement
# ----------------------------------------------------------------------------------------------
def test_declared_copies_tie_exactly_and_the_lower_id_wins():
    S = 16
    ndc = np.array([[-0.61, -0.52, 1.0], [0.63, -0.47, 1.3], [0.02, 0.71, 1.7], [-0.3, -0.3, 2.5], [0.3, -0.3, 2.5], [0.0, 0.3, 2.5]])
    faces = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2]])
    plain = shade_ref.raster_k1_detail(ndc, faces, S)
    told = shade_ref.raster_k1_detail(ndc, faces, S, dup_of=[0, 1, 1])
    hit = plain["pix_to_face"] == 1
    assert hit.sum() > 20 and (plain["pix_to_face"] != 2).all() and np.array_equal(plain["pix_to_face"], told["pix_to_face"])
    assert plain["unsure"][hit].all() and not plain["tie"].any()       # undeclared: a tie like any other
    assert not told["unsure"][hit].any() and told["tie"][hit].all() and not told["tie"][~hit].any()
    behind = hit & (told["second"] == 0)                                 # the far face 0 is the next candidate where it reaches
    assert behind.sum() > 5 and (told["second"][hit & ~behind] == -1).all()
    # the far face first, the copies after it: a pixel's tie flag does not survive a nearer winner
    rev = shade_ref.raster_k1_detail(ndc, np.array([[0, 1, 2], [3, 4, 5], [3, 4, 5]]), S, dup_of=[0, 1, 1])
    assert not rev["tie"][rev["pix_to_face"] == 0].any() and rev["tie"][rev["pix_to_face"] == 1].all()


def test_parts_of_a_cut_face_and_their_shared_diagonal():
    """One vertex behind z_clip: the winner's part index is reported, and a pixel centre on the diagonal of the quadrilateral is
    ``unsure`` (strictly inside neither part) but not ``unsure_face`` (either part is the same original face)."""
    S = 32
    ndc = np.array([[0.1, 0.2, -0.3], [-0.52, -0.41, 1.0], [0.47, -0.36, 1.2]])
    faces = np.array([[0, 1, 2]])
    parts = shade_ref.clip_mesh(ndc, faces)
    assert [q[2] for q in parts] == [0, 1]
    mid = 0.5 * (parts[0][0][0, :2] + parts[0][0][2, :2])                # p4 and p3: the diagonal
    g = shade_ref._pix_ndc(S)
    yo, xo = int(np.abs(g - mid[1]).argmin()), int(np.abs(g - mid[0]).argmin())
    moved = ndc.copy()
    moved[:, :2] += np.array([g[xo], g[yo]]) - mid
    d = shade_ref.raster_k1_detail(moved, faces, S)
    assert set(np.unique(d["part"])) == {-1, 0, 1} and ((d["part"] >= 0) == (d["pix_to_face"] == 0)).all()
    assert d["unsure"][yo, xo] and not d["unsure_face"][yo, xo]
    assert d["unsure_face"].sum() <= d["unsure"].sum() and not (d["unsure_face"] & ~d["unsure"]).any()
    whole = shade_ref.raster_k1_detail(np.array([[0.1, 0.6, 1.5], [-0.52, -0.41, 1.0], [0.47, -0.36, 1.2]]), faces, S)
    assert (whole["part"] == -1).all() and np.array_equal(whole["unsure"], whole["unsure_face"])


def test_shade_terms_and_the_float32_evaluation():
    S = 65
    verts = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    faces = np.array([[0, 1, 2]])
    R, T = _default_camera()
    R, T = R[0].numpy(), T[0].numpy()
    ndc = render_ref.project_to_ndc(torch.from_numpy(verts).float()[None], torch.from_numpy(R)[None], torch.from_numpy(T)[None],
                                    torch.tensor([60.0]))[0].numpy()
    p2f, bary, _, _ = shade_ref.raster_k1(ndc, faces, S)
    t = shade_ref.shade_terms(p2f, bary, verts, faces, R, T)
    c = int(np.flatnonzero((np.argwhere(p2f >= 0) == [S // 2, S // 2]).all(1))[0])
    for key, want in (("bsum", 1.0), ("nlen", 1.0), ("cos", 1.0), ("vr", 1.0), ("spec", 0.2)):
        assert abs(t[key][c] - want) < 1e-6, key
    back = shade_ref.shade_terms(p2f, bary[..., ::-1], verts, faces[:, ::-1], R, T)  # turned over: the same v.r, gated away
    np.testing.assert_allclose(back["vr"], t["vr"], atol=1e-12)
    assert (back["cos"] < 0).all() and (back["spec"] == 0).all()
    img64 = shade_ref.shade(p2f, bary, verts, faces, R, T, MESH_COLOR)
    img32 = shade_ref.shade(p2f, bary, verts, faces, R, T, MESH_COLOR, dtype=np.float32)
    assert img32.dtype == np.float32 and img64.dtype == np.float64
    err = np.abs(img32 - img64).max()
    assert 0.0 < err < 1e-5
    assert shade_ref.vertex_normals(verts, faces, dtype=np.float32).dtype == np.float32


# ----------------------------------------------------------------------------------------------
# the scenes of tests/test_gpu_colour_edges.py reach their branches
# ----------------------------------------------------------------------------------------------
def _hits(ref):
    return sum(int((r.pix_to_face >= 0).sum()) for r in ref)


@pytest.mark.parametrize("name", cc.SCENES)
def test_scene_exclusions_stay_under_two_percent(name):
    """Genuine near-tie / near-edge pixels plus the declared colour exclusions: at most 2 % of the scene's hit pixels.  Declared
    exact ties are compared, not excluded, and do not count."""
    s, ref = cc.get(name), cc.reference(name)
    assert s.N <= 6 and s.verts_ndc.dtype == np.float32 and s.verts_world.shape[0] * s.views == s.N
    out = sum(int((r.unsure | r.excluded).sum()) for r in ref)
    assert _hits(ref) > 0 and out <= 0.02 * _hits(ref), (out, _hits(ref))
    for r in ref:
        assert np.isfinite(r.image).all() and np.isfinite(r.image32).all()


@pytest.mark.parametrize("name", [f"partial{S}" for S in cc.PARTIAL_SIZES] + ["size516"])
def test_partial_tile_scenes_hit_the_last_row_and_column(name):
    s, r = cc.get(name), cc.reference(name)[0]
    edge = cc.TILE * (s.S // cc.TILE)
    assert s.S % cc.TILE != 0
    sure = (r.pix_to_face >= 0) & ~r.unsure
    assert sure[:, edge:].any() and sure[edge:, :].any() and sure[:edge, :edge].any()
    assert (r.pix_to_face < 0).any()


def test_overflow_scenes_exceed_their_lists_twice_over():
    for name in ("overflow", "ties_overflow"):
        s = cc.get(name)
        cap = cc.list_cap(s.F, s.S)
        assert cap == 8 * s.F
        assert cc.tile_entries(s.verts_ndc[0], s.faces, s.S).sum() >= 2 * cap          # (counted without the kernel's 0.01 px of slack)
        assert 2 * cc.tile_entries(s.verts_ndc[1], s.faces, s.S, slack=0.01).sum() <= cap  # the image beside it is binned
        assert cc.tile_entries(s.verts_ndc[1], s.faces, s.S).max() > 64                 # ... with lists of several batches
    s = cc.get("ties_overflow")
    pairs = [np.flatnonzero(s.dup_of == k) for k in range(s.F // 2)]
    assert all(len(p) == 2 and p[0] // 64 != p[1] // 64 for p in pairs)                 # the copies sit in different 64-face groups


def test_sizes_above_512_are_never_binned():
    for S in (520, 516):
        s = cc.get(f"size{S}")
        tiles_x = -(-S // cc.TILE)
        assert tiles_x == 65 and tiles_x * tiles_x > cc.COUNT_TILES_MAX and cc.list_cap(s.F, S) == 0 and tiles_x <= 256
        assert s.F <= 300
    assert cc.list_cap(168, 512) == 16 * 168 and cc.list_cap(168, 256) == 8 * 168


@pytest.mark.parametrize("name", cc.TIES)
def test_tie_scenes_tie_on_every_hit(name):
    s, ref = cc.get(name), cc.reference(name)
    F = s.F
    assert np.array_equal(s.faces[np.arange(F)], s.faces[s.dup_of]) and (s.dup_of <= np.arange(F)).all()
    assert (np.bincount(s.dup_of, minlength=F)[np.unique(s.dup_of)] == 2).all()
    for r in ref:
        hit = r.pix_to_face >= 0
        assert np.array_equal(r.tie, hit)                                              # every hit is a tie of two copies
        assert np.array_equal(s.dup_of[r.pix_to_face[hit]], r.pix_to_face[hit])      # ... that the lower id wins
        assert len(np.unique(r.pix_to_face[hit])) >= 3
    if name != "ties_overflow":
        tx, ty = cc.STACK_TILE
        entries = cc.tile_entries(s.verts_ndc[0], s.faces, s.S)
        assert entries[ty, tx] == F and entries.sum() <= cc.list_cap(F, s.S)
        assert F <= 64 if name == "ties_batch" else F > 128
    if name == "ties_permuted":
        # a tile's list holds the even ids before the odd ones (two copies of the setup's counters): pairs (odd, even) read the higher
        # id first; and pairs 64 or more ids apart cannot share a batch
        win = np.unique(ref[0].pix_to_face[ref[0].pix_to_face >= 0])
        other = np.array([int(np.flatnonzero((s.dup_of == k) & (np.arange(F) != k))[0]) for k in win])
        assert ((win % 2 == 1) & (other % 2 == 0)).any() and ((win % 2 == 0) | (other % 2 == 1)).any()


@pytest.mark.parametrize("name", cc.STACKS)
def test_stack_scenes_have_their_batch_sizes(name):
    s, r = cc.get(name), cc.reference(name)[0]
    n = int(name[5:].split("_")[0])
    tx, ty = cc.STACK_TILE
    for slack in (0.0, 0.01):
        entries = cc.tile_entries(s.verts_ndc[0], s.faces, s.S, slack)
        assert entries[ty, tx] == n == s.F and entries.sum() <= cc.list_cap(s.F, s.S)   # binned, n entries on the tile
    z = s.verts_ndc[0][s.faces][..., 2].astype(np.float64)
    order = np.argsort(z.min(1))
    assert (z.min(1)[order][1:] / z.max(1)[order][:-1] - 1.0 >= 1e-3).all()             # depths at least 1e-3 apart
    tile = r.pix_to_face[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
    if name.endswith("partial"):
        assert order[0] == 0 and order[1] == n - 1
        assert 5 <= (tile == 0).sum() <= 32 and ((tile == 0) | (tile == n - 1)).all()
    else:
        assert order[0] == (0 if name.endswith("near") else n - 1) and (tile == order[0]).all()
    assert not r.unsure[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].any()


def test_cut_scene_compares_front_parts_of_both_kinds():
    s, ref = cc.get("cuts"), cc.reference("cuts")
    nb = s.info["n_behind"]
    assert sorted(set(nb.tolist())) == [1, 2]
    for c, r in enumerate(ref):
        z = s.verts_ndc[c][s.faces][..., 2]
        assert np.array_equal((z[0] < shade_ref.Z_CLIP), np.arange(3) == c)             # face 0: corner c behind
        assert np.array_equal((z[1] < shade_ref.Z_CLIP), np.arange(3) != c)             # face 1: corner c alone in front
        sure = (r.pix_to_face >= 0) & ~r.unsure
        assert ((r.part >= 0) == (r.pix_to_face >= 0)).all()                             # every winner is a front part
        for kind, parts in ((1, {0, 1}), (2, {0})):
            mine = sure & np.isin(r.pix_to_face, np.flatnonzero(nb == kind))
            assert mine.sum() >= 50 and set(np.unique(r.part[mine])) == parts, (c, kind, mine.sum())
        for f in (0, 1):  # the map-back shows: position and shading vary over the compared part pixels by far more than the bound
            px = sure & (r.pix_to_face == f)
            assert np.ptp(r.image[2][px]) > 100 * 2e-4
            assert (r.bary[px] > 1e-3).all() and np.ptp(r.bary[px], axis=0).min() > 0.02


def test_shading_scenes_show_their_terms():
    r = cc.reference("specular")[0]
    sure = ~r.unsure[r.pix_to_face >= 0]
    spec = r.terms["spec"][sure]
    assert (spec > 0.05).sum() >= 20 and ((spec > 1e-4) & (spec < 1e-2)).sum() >= 20 and (r.terms["cos"] > 0).all()
    b = cc.reference("backfacing")[0]
    assert (b.terms["cos"] < 0).all() and (b.terms["spec"] == 0).all()
    assert (0.2 * np.maximum(b.terms["vr"], 0.0) ** 64 > 0.05).sum() >= 20               # what a missing gate would add
    hit = b.pix_to_face >= 0
    np.testing.assert_allclose(b.image[:, hit], 0.5 * np.asarray(cc.RGB)[:, None] * b.terms["bsum"][None], rtol=0, atol=1e-15)


def test_degenerate_scene_has_its_three_features():
    s, r = cc.get("degenerate"), cc.reference("degenerate")[0]
    assert s.info["unused_vertex"] not in s.faces
    for dtype in (np.float64, np.float32):
        n = shade_ref.vertex_normals(s.verts_world[0], s.faces, dtype=dtype)
        assert (n[[0, 1, s.info["unused_vertex"], 9]] == 0).all()                         # opposite equal normals cancel exactly; no face; no area
        np.testing.assert_allclose(np.linalg.norm(n[[2, 3, 5, 6, 7, 8]], axis=1), 1.0, atol=1e-6)
    assert (n[7] == -n[8]).all() and np.abs(n[[5, 6]] - n[7]).max() < 1e-6             # the larger face decides the shared edge's normals
    won = np.unique(r.pix_to_face[r.pix_to_face >= 0])
    assert set(won) == set(range(s.F)) - set(s.info["no_area"])
    small = r.pix_to_face == 4                                                           # the interpolated normal changes sign inside it
    cos = np.zeros(r.pix_to_face.shape)
    cos[r.pix_to_face >= 0] = r.terms["cos"]
    assert (cos[small] > 0.1).any() and (cos[small] < -0.1).any()
    nlen = np.ones(r.pix_to_face.shape)
    nlen[r.pix_to_face >= 0] = r.terms["nlen"]
    assert nlen[np.isin(r.pix_to_face, [0, 1, 4])].min() < 0.05                         # ... and gets short on the way (and along edge a-b)


def test_camera_scene_tells_its_cameras_apart():
    """Shaded through camera 0 instead of its own, every other image moves by more than ten times the colour bound."""
    for name, others in (("cameras_N", range(1, 6)), ("cameras_views", (1, 3, 5))):
        s, ref = cc.get(name), cc.reference(name)
        assert s.views == 2 and s.N == 6 and len(s.R) == len(s.T) == len(s.fov) == len(s.aspect) == {"cameras_N": 6, "cameras_views": 2}[name]
        for n in others:
            r = ref[n]
            wrong = shade_ref.shade(r.pix_to_face, r.bary, s.verts_world[n // 2], s.faces, s.R[0], s.T[0], cc.RGB)
            sure = (r.pix_to_face >= 0) & ~r.unsure
            assert np.abs(wrong - r.image)[:, sure].max() > 10 * 2e-4
    one = cc.get("cameras_1")
    assert len(one.R) == len(one.T) == 1 and np.array_equal(one.verts_ndc[0], one.verts_ndc[1])
