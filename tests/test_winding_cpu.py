"""CPU-side checks of the winding numbers: the library's new surface, the restatement (tests/winding_ref.py) that the GPU tests compare
the kernel with - pinned to hand cases with exact answers, in float64 and in float32 - and the conditions under which the GPU tests'
cases (tests/winding_cases.py) mean what they say."""
import os
import re

import numpy as np
import pytest

import point_mesh_cases as PC
import point_mesh_ref as PR
import winding_cases as WC
import winding_ref as WR
from conftest import REPO

DTYPES = [np.float64, np.float32]
EPS = {np.float64: 2.0 ** -50, np.float32: 2.0 ** -22}  # a few roundings of values <= 1


def test_library_surface():
    from smilify_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "smil_point_mesh_winding")
    v = lib.smil_version()
    assert b"0.12" in v and b"winding numbers" in v, v
    header = open(os.path.join(REPO, "include", "smilfit.h")).read()
    comment = header[header.index("smil_point_mesh_winding: "):header.index("size_t smil_point_mesh_workspace_bytes")]
    for words in ("det == 0", "NaN", "without faces gives 0", "atan2(det, den)", "int64 fixed point"):
        assert words in comment, words
    # bad arguments are refused before anything is launched, with smil_point_face_distance's conventions
    assert lib.smil_point_mesh_winding(None, 1, None, None, 1, 1, 1, None, 1, None, 0, None, None, None) == -1
    assert b"null argument" in lib.smil_last_error()


def test_python_surface_without_gpu():
    from smilify_amd import engine, fit3d, mesh3d

    assert callable(engine.point_mesh_winding)
    for name in ("winding_number", "contains", "signed_distance"):
        assert callable(getattr(mesh3d, name))
    for name in ("point_mesh_signed_distance", "containment_loss", "penetration_loss"):
        assert callable(getattr(fit3d, name))
    assert mesh3d.SignedDistance._fields == ("sdist", "dist2", "face", "bary", "points", "winding")
    assert "w_contain" not in fit3d.default_weights
    assert fit3d.build_parser().parse_args(["--mesh_dir", "x"]).w_contain == 0.0
    assert fit3d.build_parser().parse_args(["--mesh_dir", "x", "--w_contain", "2"]).w_contain == 2.0


def test_integer_sum_unit_is_the_librarys():
    """fix_unit_exp of csrc/common.h, read from the source, with the addend bound 0.5 (eb = 0) and F addends; the kernel names it."""
    src = open(os.path.join(REPO, "smilify_amd", "csrc", "common.h")).read()
    body = re.search(r"int fix_unit_exp\(int eb, long long addends\) \{ return (.+?); \}", src).group(1)
    assert body == "61 - (64 - __clzll(addends)) - eb"
    clz = lambda x: 64 - int(x).bit_length()  # noqa: E731
    for F in (1, 2, 3, 127, 128, 129, 1280, 10878, 2 ** 20, 2 ** 29 - 1):
        assert WR.fix_exp(F) == 61 - (64 - clz(F)) - 0
        assert 0.5 * 2.0 ** WR.fix_exp(F) * F < 2.0 ** 62
    assert WR.fix_exp(0) == WR.fix_exp(1) == 60
    kernel = open(os.path.join(REPO, "smilify_amd", "csrc", "point_mesh.hip")).read()
    assert "fix_unit_exp(0, max(m.F, 1))" in kernel


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_cases(dtype):
    eps = EPS[dtype]
    assert abs(WR.pair_value(WC.OCTANT, [0, 0, 0], dtype) - 0.125) <= eps
    assert abs(WR.pair_value(WC.OCTANT[::-1], [0, 0, 0], dtype) + 0.125) <= eps  # the orientation gives the sign
    assert abs(WR.winding(np.asarray(WC.OCTANT, np.float32), [[0, 1, 2]], [[0, 0, 0]], dtype)[0] - 0.125) <= eps
    v, f = WC.cube()
    for t in f:
        assert abs(WR.pair_value(v[t], [0, 0, 0], dtype) - 1.0 / 12.0) <= eps
    inside, outside = [[0, 0, 0], [0.25, -0.5, 0.75]], [[3, 0.25, 0.125], [-1.5, 1.5, 1.5]]
    assert np.abs(WR.winding(v, f, inside, dtype) - 1.0).max() <= 12 * eps
    assert np.abs(WR.winding(v, f, outside, dtype)).max() <= 12 * eps
    assert np.abs(WR.winding(*WC.cube(flip=True), inside, dtype) + 1.0).max() <= 12 * eps
    assert np.abs(WR.winding(*WC.nested_cubes(), [[0, 0, 0], [0.25, 0.125, -0.25]], dtype) - 2.0).max() <= 24 * eps
    assert abs(WR.winding(*WC.nested_cubes(), [[0.75, 0, 0]], dtype)[0] - 1.0) <= 24 * eps
    assert abs(WR.winding(*WC.cube(top=False), [[0, 0, 0]], dtype)[0] - 5.0 / 6.0) <= 12 * eps


@pytest.mark.parametrize("dtype", DTYPES)
def test_det_zero_adds_exactly_zero(dtype):
    tri = np.asarray(PC.TRI, np.float32)
    for p in ([0.25, 0.25, 0.0], [2.0, 3.0, 0.0], [-1.0, 0.5, 0.0],  # in the plane: inside the face and outside
              [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],  # on a vertex
              [0.5, 0.5, 0.0], [0.5, 0.0, 0.0]):  # on an edge
        assert WR.pair_value(tri, p, dtype) == 0.0, p
        assert WR.winding(tri, [[0, 1, 2]], [p], dtype)[0] == 0.0, p
    for _, t, p, _, _ in PC.DEGENERATE:
        assert WR.pair_value(t, p, dtype) == 0.0
        assert WR.pair_value(t, [0.3, -0.7, 0.2], dtype) == 0.0
    # a point on a vertex of a closed mesh: the faces around it add 0, the others what they subtend, and no NaN
    v, f = WC.cube()
    w = WR.winding(v, f, v, dtype)
    assert np.isfinite(w).all() and np.abs(w - 0.125).max() <= 12 * EPS[dtype]


def test_unusable_faces_points_and_empty_meshes():
    v, f = WC.cube()
    assert WR.winding(v, f[:0], [[0, 0, 0]])[0] == 0.0
    bad = v.copy()
    bad[7, 1] = np.nan
    less = WR.winding(bad, f, [[0, 0, 0]])[0]
    assert abs(less - (1.0 - (f == 7).any(1).sum() / 12.0)) <= 1e-14
    out_of_range = f.copy()
    out_of_range[0, 2] = 8
    assert abs(WR.winding(v, out_of_range, [[0, 0, 0]])[0] - 11.0 / 12.0) <= 1e-14
    w = WR.winding(v, f, [[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 3.3e38]])
    assert w[0] == 1.0 and np.isnan(w[1:]).all()
    # scaling by a power of two and permuting the faces: the same bits, in float32 too
    p = PC.random_cloud(3, 50)
    sv, sf = WC.soup()
    base = WR.winding(sv, sf, p, np.float32)
    perm = np.random.default_rng(4).permutation(len(sf))
    assert np.array_equal(base, WR.winding(sv, sf[perm], p, np.float32))
    for s in (2.0 ** 20, 2.0 ** -20):
        assert np.array_equal(base, WR.winding(sv * np.float32(s), sf, p * np.float32(s), np.float32))


def _distance64(v, f, p):
    return PR.point_face(v, f, p)[0].sqrt().numpy()


@pytest.mark.parametrize("name", WC.NAMES)
def test_cases_are_decided_and_float32_decides_them(name):
    """What the GPU tests rely on: no generated point has a float64 winding number within BAND of 0.5, and the float32 restatement
    alone makes the float64 decision for every point at least 2^-14 E from the surface."""
    v, f, p = WC.case(name)
    assert p.shape == (WC.NEAR + WC.BOX, 3) and p.dtype == np.float32
    w64, w32 = WR.winding(v, f, p, np.float64), WR.winding(v, f, p, np.float32)
    assert np.isfinite(w64).all() and float(np.abs(w64 - 0.5).min()) >= WC.BAND
    differ = np.nonzero((w32 > 0.5) != (w64 > 0.5))[0]
    if len(differ):
        d = _distance64(v, f, p[differ])
        assert (d < WC.DECIDED_FROM * WC.extent(v, p)).all(), (name, differ.tolist(), d.tolist())
    print(f"\n[winding] {name}: faces={len(f)} inside={int((w64 > 0.5).sum())} float32-vs-float64 max error "
          f"{float(np.abs(w32 - w64).max()):.3g}, decisions that differ {len(differ)}, range {w64.min():.3f} .. {w64.max():.3f}")


def test_hull_case_is_valid():
    """The small carve: no voxel centre near a face, and fewer than half of the voxels have a mixed neighbourhood."""
    occ, centres, same = WC.hull_occupancy().reshape(-1), WC.hull_centres(), WC.hull_uniform_neighbourhood()
    assert len(centres) == WC.HULL_G ** 3 <= 16 ** 3 and 0 < occ.sum() < len(occ)
    left_out = 1.0 - same.mean()
    print(f"\n[winding] hull: voxels left out after relaxation {left_out:.3f}")
    assert left_out < 0.5
    for taubin, which in ((0, np.ones_like(same)), (4, same)):
        v, f = WC.hull_mesh(taubin)
        w = WR.winding(v, f, centres[which])
        assert np.array_equal(w > 0.5, occ[which] != 0), taubin
        assert float(np.abs(w - np.rint(w)).max()) < 1e-9  # closed and oriented: an integer for every centre
