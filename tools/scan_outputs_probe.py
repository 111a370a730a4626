"""Every output of the entry points behind the tiled all-pairs scans (csrc/scan.h) from seeded inputs, as one .npz: run once per build
of the library (``SMILFIT_LIB`` selects one, smilify_amd/_lib.py), each in its own process, and compare the two files as raw bytes,
so that NaNs compare too.  For changes to scan.h, mesh3d.hip, raycast.hip, point_mesh.hip, point_mesh.h and mesh_bvh.hip that must
not change a single bit: the keys merge with integer atomics and the sums are fixed point, so two builds that compute the same
thing agree exactly.

    SMILFIT_LIB=/path/to/parent/libsmilfit.so python3 tools/scan_outputs_probe.py --out /tmp/scan_a.npz
    python3 tools/scan_outputs_probe.py --out /tmp/scan_b.npz
    python3 tools/scan_outputs_probe.py --compare /tmp/scan_a.npz /tmp/scan_b.npz

Covers smil_chamfer at (1, 4100, 4100) both ways and single-directional (four splits, the last one short); smil_knn and
smil_sdf_distance at K = 1, 5, 64 on (2, 300, 700); smil_ray_diameters at F = 3 * 256 + 28 faces and 100 rays a sample (four
tiles, the last one short); smil_point_face_distance, smil_face_point_distance and smil_point_mesh_winding on two meshes of 700
and 450 faces and clouds of 300 points, one padded and one with a NaN point, with ``splits`` 0, 1 and 3, the backward of both
directions, and smil_bvh_point_face_distance on the same meshes.  A few seconds in all.
"""
import argparse
import os
import sys

import numpy as np
import probelib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="the .npz the arrays are written to")
ap.add_argument("--compare", nargs=2, metavar="NPZ", help="compare two such files instead of running anything")
args = ap.parse_args()

if args.compare:
    a, b = (probelib.load_arrays(p) for p in args.compare)
    only, changed = probelib.differing(a, b)
    bad = [("only in one file", n) for n in only] + [(n, str(a[n].dtype), a[n].shape, b[n].shape) for n in changed]
    print(f"{len(a)} / {len(b)} arrays, byte for byte: {len(bad)} differ")
    for x in bad:
        print("DIFFERS", x)
    sys.exit(1 if bad or not a else 0)

import torch  # noqa: E402

from smilify_amd import engine as eng  # noqa: E402

DEV = "cuda:0"
out = {}


def save(tag, names, values):
    for k, v in zip(names, values):
        if v is not None:
            out[f"{tag}.{k}"] = v.detach().cpu().numpy()


def clouds(N, P1, P2, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, P1, 3, generator=g).to(DEV), (torch.randn(N, P2, 3, generator=g) * 1.1 + 0.05).to(DEV)


def soup(sizes, seed):
    """Packed meshes of random small triangles in [-1, 1]^3: (verts, MeshTables)."""
    g = torch.Generator().manual_seed(seed)
    verts, faces, f_off, v_off = [], [], [0], [0]
    for F in sizes:
        c = torch.rand(F, 1, 3, generator=g) * 2 - 1
        verts.append((c + 0.15 * torch.randn(F, 3, 3, generator=g)).reshape(-1, 3))
        faces.append(torch.arange(3 * F).reshape(F, 3) + v_off[-1])
        f_off.append(f_off[-1] + F)
        v_off.append(v_off[-1] + 3 * F)
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32).contiguous().to(DEV)  # noqa: E731
    mt = eng.MeshTables(i32(torch.cat(faces)), i32(f_off), i32(v_off), len(sizes), f_off[-1], max(sizes), v_off[-1], 3 * max(sizes))
    return torch.cat(verts).contiguous().to(DEV), mt


def run_chamfer():
    x, y = clouds(1, 4100, 4100, 1)
    for single in (False, True):
        save(f"chamfer.single{int(single)}", ("loss", "idx_x", "idx_y", "d_x", "d_y"), eng.chamfer(x, y, single_directional=single))


def run_knn_sdf():
    x, y = clouds(2, 300, 700, 2)
    g = torch.Generator().manual_seed(3)
    xs, ys = torch.randn(2, 300, generator=g).to(DEV), torch.randn(2, 700, generator=g).to(DEV)
    for K in (1, 5, 64):
        save(f"knn.K{K}", ("dists_x", "idx_x", "dists_y", "idx_y", "insertions"), eng.knn(x, y, K, both=True))
        loss, d_x, d_y, tables, ins = eng.sdf_distance(x, y, xs, ys, K, want_tables=True)
        save(f"sdf.K{K}", ("loss", "d_x", "d_y", "insertions") + tuple(f"table{i}" for i in range(4)), (loss, d_x, d_y, ins) + tables)


def run_rays():
    F, S, R = 3 * 256 + 28, 64, 100
    verts, mt = soup([F], 4)
    g = torch.Generator().manual_seed(5)
    own = torch.randint(0, F, (S,), generator=g).to(torch.int32).to(DEV)
    origins = verts[mt.faces[own.long()].long()].mean(1).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn(S, R, 3, generator=g), dim=2).to(DEV)
    save("rays", ("diam", "ray_t"), eng.ray_diameters(verts, mt.faces, origins, own, dirs, 1e-4, 1e-3, 3.0, 20, want_ray_t=True))


def run_point_mesh():
    verts, mt = soup([700, 450], 6)
    g = torch.Generator().manual_seed(7)
    points = (torch.rand(2, 300, 3, generator=g) * 2.4 - 1.2).to(DEV)
    points[0, 17, 1] = float("nan")
    lengths = torch.tensor([300, 211], dtype=torch.int32, device=DEV)
    for splits in (0, 1, 3):
        for by_face in (False, True):
            tag = f"pm.splits{splits}.by_face{int(by_face)}"
            dist2, idx, bary = eng.point_mesh_distance(verts, mt, points, lengths, by_face=by_face, splits=splits)
            save(tag, ("dist2", "idx", "bary"), (dist2, idx, bary))
            gup = torch.randn(dist2.shape, generator=g).to(DEV)
            save(tag + ".bwd", ("d_points", "d_verts"), eng.point_mesh_backward(verts, mt, points, lengths, idx, gup, by_face=by_face))
        save(f"winding.splits{splits}", ("w",), (eng.point_mesh_winding(verts, mt, points, lengths, splits=splits),))
    order, boxes = eng.bvh_build(verts, mt)
    save("bvh", ("order", "boxes"), (order, boxes))
    for sort in (False, True):
        res = eng.bvh_point_face_distance(verts, mt, order, boxes, points, lengths, sort_queries=sort, want_evaluated=True)
        save(f"bvh.sorted{int(sort)}", ("dist2", "face", "bary", "evaluated"), res)


for step in (run_chamfer, run_knn_sdf, run_rays, run_point_mesh):
    step()
    torch.cuda.synchronize()
    print(f"{step.__name__}: {len(out)} arrays so far", flush=True)
np.savez(args.out, **out)
print(f"{len(out)} arrays in {args.out} (library: {os.environ.get('SMILFIT_LIB', 'the default build')})")
