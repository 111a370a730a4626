"""CPU-side checks of the mesh hierarchy: the header declares the calls and the derived binding loads them, and the numpy restatement
tests/mesh_bvh_ref.py of the traversal - exact boxes, nearer child first, the key {d^2, face}, a node entered when its box distance is
<= the limit with its margin - reproduces the sequential scan on the cases where every answer is a tie.  The two wrong rules (a
strict <; no margin) are run as well, so that the cases are known to tell them apart where they can."""
import os

import numpy as np
import torch

import mesh_bvh_cases as BC
import mesh_bvh_ref as BR
import point_mesh_cases as PC
import point_mesh_ref as PR
import winding_cases as WC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("smil_bvh_workspace_bytes", "smil_bvh_nodes", "smil_bvh_codes", "smil_bvh_build", "smil_bvh_refit", "smil_bvh_point_codes",
         "smil_bvh_point_face_distance")


def test_header_binding_and_sources():
    from smilify_amd import _lib

    header = open(os.path.join(REPO, "include", "smilfit.h")).read()
    lib = _lib.load()
    for name in CALLS:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name), name
    assert _lib.BVH_LEAF == BC.leaf_size() >= 2 and _lib.BVH_SENTINEL == BR.SENTINEL == 1 << 30
    v = lib.smil_version()
    assert b"0.13" in v and b"mesh BVH" in v, v
    assert lib.smil_bvh_workspace_bytes(0, 1, 1, 1) == 0 and lib.smil_bvh_nodes(1, 0) == 0
    assert lib.smil_bvh_workspace_bytes(2, 100, 50, 60) > lib.smil_point_mesh_workspace_bytes(2, 100, 50, 60)
    assert lib.smil_bvh_nodes(2, 100) == 4 * (100 // _lib.BVH_LEAF + 2)
    # the search's frame, table and finish exist once: the hierarchy includes them, it does not restate them
    csrc = os.path.join(REPO, "smilify_amd", "csrc")
    bvh, shared = open(os.path.join(csrc, "mesh_bvh.hip")).read(), open(os.path.join(csrc, "point_mesh.h")).read()
    assert '#include "point_mesh.h"' in bvh and '#include "point_mesh.h"' in open(os.path.join(csrc, "point_mesh.hip")).read()
    for name in ("k_pm_finish", "k_pm_table", "k_pm_extent", "closest_on_triangle(T"):
        assert "void " + name not in bvh and name + "(T" not in bvh, name
    assert "pm_prepare(" in bvh and "pm_finish(" in bvh and "int pm_prepare(" in shared and "mesh_bvh.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "2^-18" in bvh and "2^-19" in bvh  # the margin the restatement uses
    assert BR.EPS == np.float32(2.0 ** -18) and BR.SLACK == np.float32(1 + 2.0 ** -19)


def test_python_surface_without_gpu():
    import inspect

    from smilify_amd import fit3d, mesh3d

    for fn in (mesh3d.closest_points, mesh3d.signed_distance, fit3d.point_face_distance, fit3d.point_mesh_signed_distance,
               fit3d.containment_loss, fit3d.penetration_loss):
        p = inspect.signature(fn).parameters["bvh"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    assert all(hasattr(mesh3d.MeshBVH, m) for m in ("refit", "closest_points", "arrays"))


def _ties(name):
    if name == "copies":
        verts, faces = BC.copies(300)
        return verts, faces, np.round(PC.random_cloud(31, 65, 1.0) * 8) / 8
    if name == "lattice":
        return BC.lattice(32)
    if name == "tie fan":
        return PC.tie_fan()[:3]
    if name == "hull":
        import hull_mesh_ref as MR

        occ = BC.hull_occupancy()
        m = MR.extract(occ, WC.HULL_ORIGIN, WC.HULL_VOXEL, (), want_normals=False)
        return m.verts.astype(np.float32), m.faces.astype(np.int64), BC.voxel_centres(occ, WC.HULL_ORIGIN, WC.HULL_VOXEL)
    verts, faces, points = PC.hand_mesh(PC.HAND + PC.DEGENERATE)
    return verts, faces, points


def _sequential(verts, faces, points):
    """point_mesh_ref.point_face on the case (float64): on these inputs every product is exact, so its first minimum is the float32
    scan's."""
    d2, face = PR.point_face(verts, faces, torch.from_numpy(np.asarray(points, np.float64)))
    return d2.numpy(), face.numpy()


def test_restated_traversal_reproduces_the_sequential_scan_on_ties():
    leaf = BC.leaf_size()
    wrong = {}
    for name in ("copies", "lattice", "tie fan", "hull", "hand"):
        verts, faces, points = _ties(name)
        tree = BR.build(verts, faces, leaf)
        assert sorted(tree["order"].tolist()) == list(range(len(faces)))
        d2, face, count = BR.query(tree, verts, faces, points)
        want_d2, want_face = _sequential(verts, faces, points)
        sh = BR.frame_shift(verts, faces, points)
        b_d2, b_face = BR.brute(verts, faces, points)
        assert np.array_equal(b_face, face) and np.array_equal(b_d2, d2), name  # the float32 scan with a strict <, always
        if name == "hull":
            # a surface-nets vertex is a mean of three or more edge points: not dyadic, so float32 and float64 break other ties
            # and point_face's indices are not the float32 scan's here (tests/test_gpu_point_mesh.py says the same of the kernel);
            # the float32 scan above stands in
            want_face = b_face
            assert (np.abs(np.ldexp(d2.astype(np.float64), -2 * sh) - want_d2) <= 8 * PR.U * np.maximum(want_d2, 2.0 ** (-2 * sh - 24))).all()
        else:
            assert np.array_equal(face, want_face), (name, int((face != want_face).sum()))
        if name not in ("copies", "hull"):  # (copies: the parameters are quotients like 1 / 3, rounded differently in float32)
            assert np.array_equal(np.ldexp(d2.astype(np.float64), -2 * sh), want_d2), name
        assert count.min() >= 1 and count.max() <= len(faces)
        if name == "copies":
            assert (face == 0).all()
        if name == "lattice":  # on the surface best is 0 once the point's own cell is met: only boxes that touch the point are entered
            assert count.mean() < len(faces) / 8, (name, count.mean())
        # on these exact inputs the <= rule alone finds every tie's smallest face (the margin is for rounding) ...
        assert np.array_equal(BR.query(tree, verts, faces, points, margin=False)[1], want_face), name
        strict = BR.query(tree, verts, faces, points, margin=False, tie_rule=False)[1]
        wrong[name] = int((strict != want_face).sum())
    # ... and entering a node only when D^2 < best loses it: the cases must show that
    assert wrong["lattice"] > 0 and wrong["hull"] > 0, wrong


def test_restated_build_matches_its_own_invariants():
    leaf = BC.leaf_size()
    verts, faces = PC.random_mesh(61, 80, 1000, degenerate=True)
    verts = verts.copy()
    verts[3] = np.nan
    tree = BR.build(verts, faces, leaf)
    ok, tri = BR.usable_faces(verts, faces)
    order, Lp, boxes = tree["order"], tree["Lp"], tree["boxes"]
    assert tree["L"] == 125 and Lp == 128 and not ok[order[int(ok.sum()):]].any() and ok[order[:int(ok.sum())]].all()
    assert np.isinf(boxes[Lp + 125:]).all()
    root = boxes[1]
    assert np.array_equal(root[:3], tri[ok].min((0, 1))) and np.array_equal(root[3:], tri[ok].max((0, 1)))
    # a refit on displaced vertices keeps the order and answers like the scan
    rng = np.random.default_rng(5)
    moved = (verts + 0.3 * rng.standard_normal(verts.shape)).astype(np.float32)
    L, Lp2, boxes2 = BR.boxes_of(moved, faces, order, leaf)
    refit = dict(tree, boxes=boxes2)
    points = PC.random_cloud(6, 64)
    d2, face, _ = BR.query(refit, moved, faces, points)
    b_d2, b_face = BR.brute(moved, faces, points)
    assert np.array_equal(face, b_face) and np.array_equal(d2, b_d2)
