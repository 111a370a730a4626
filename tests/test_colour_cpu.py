"""CPU checks of the colour (HardPhong) path: the C ABI declares, exports and binds it, and the float64 restatement the GPU tests
judge it by (tests/shade_ref.py) gives hand-computed answers."""
import os
import re

import numpy as np
import torch

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
