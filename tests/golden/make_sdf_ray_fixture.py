"""Writes tests/golden/sdf_ray_ref.npz: the reference's own compute_sdf, smooth_distances and assign_vertex_sdf
(fitter_3d/SDF_tests.py) on a small closed mesh, in float32 on the CPU as the reference runs them.

    python tests/golden/make_sdf_ray_fixture.py /path/to/reference/checkout

The reference module is imported with ``pytorch3d``, ``matplotlib``, ``psutil``, ``GPUtil`` and ``config`` stubbed (none is needed by
the three functions); the ``Meshes`` stub offers ``verts_packed``, ``faces_packed``, ``faces_areas_packed`` and ``device``.
``generate_random_directions_batch`` is wrapped to record what it returned, and ``torch.multinomial`` to record the
sampled faces (the points are the function's own return value).  The mesh is a torus whose tube narrows to a neck, 16 x 10 quads =
320 triangles, built here.  Two runs: all-faces mode (320 samples, cap 160: never reached with 30 rays), and a sampled mode with
``num_samples = 12`` whose cap of 6 valid rays bites.  The file holds data only.
"""
import os
import sys
import time
import types

import numpy as np
import torch

NUM_RAYS = 30
SAMPLED = 12
K_SMOOTH = (10, 5)   # all-faces, sampled
K_VERTEX = (10, 4)
SEED = 20


class Meshes:
    def __init__(self, verts, faces):
        self._v, self._f = verts[0], faces[0]
        self.device = self._v.device

    def verts_packed(self):
        return self._v

    def faces_packed(self):
        return self._f

    def faces_areas_packed(self):
        fv = self._v[self._f]
        return 0.5 * torch.norm(torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1), dim=1)


def import_reference(root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("pytorch3d")
    stub("pytorch3d.ops")
    stub("pytorch3d.ops.knn", knn_points=None)
    stub("pytorch3d.io", load_obj=None)
    stub("pytorch3d.structures", Meshes=Meshes)
    mpl = stub("matplotlib", use=lambda *_a, **_k: None)
    mpl.pyplot = stub("matplotlib.pyplot")
    mpl.tri = stub("matplotlib.tri", Triangulation=None)
    stub("psutil")
    stub("GPUtil")
    stub("config")
    sys.path.insert(0, root)
    import fitter_3d.SDF_tests as m

    return m


def neck_torus(nu=16, nv=10):
    """A torus of major radius 1 whose tube radius varies 0.38 .. 0.14 around the ring; float32 vertices, outward faces."""
    u = 2 * np.pi * (np.arange(nu) + 0.13) / nu
    v = 2 * np.pi * (np.arange(nv) + 0.29) / nv
    r = 0.26 + 0.12 * np.cos(u)
    uu, rr = np.repeat(u, nv), np.repeat(r, nv)
    vv = np.tile(v, nu)
    verts = np.stack([(1.0 + rr * np.cos(vv)) * np.cos(uu), (1.0 + rr * np.cos(vv)) * np.sin(uu), rr * np.sin(vv)], 1)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            faces += [[a, b, d], [a, d, c]]
    return verts.astype(np.float32), np.asarray(faces, np.int64)


def run(ref, verts, faces, num_samples, k_smooth, k_vertex):
    rec = dict(dirs=[], face_idx=None)
    orig_dirs, orig_multinomial = ref.generate_random_directions_batch, torch.multinomial

    def dirs_wrap(normals, num_rays, device):
        d = orig_dirs(normals, num_rays, device)
        rec["dirs"].append(d.clone())
        return d

    def multinomial_wrap(*a, **k):
        rec["face_idx"] = orig_multinomial(*a, **k)
        return rec["face_idx"]

    ref.generate_random_directions_batch, torch.multinomial = dirs_wrap, multinomial_wrap
    try:
        torch.manual_seed(SEED)
        mesh = Meshes([torch.from_numpy(verts)], [torch.from_numpy(faces)])
        t0 = time.perf_counter()
        points, diam = ref.compute_sdf(mesh, num_samples=num_samples, num_rays=NUM_RAYS)
        print(f"reference compute_sdf(num_samples={num_samples}): {time.perf_counter() - t0:.2f} s on this CPU")
    finally:
        ref.generate_random_directions_batch, torch.multinomial = orig_dirs, orig_multinomial
    smoothed = ref.smooth_distances(points, diam, k=k_smooth)
    vertex = ref.assign_vertex_sdf(torch.from_numpy(verts), points, smoothed, k=k_vertex)
    face_idx = rec["face_idx"].numpy() if rec["face_idx"] is not None else np.arange(len(faces))
    return dict(points=points.numpy(), face_idx=face_idx.astype(np.int64), dirs=torch.cat(rec["dirs"]).numpy(), diam=diam.numpy(),
                smoothed=smoothed.numpy(), vertex_sdf=vertex.numpy(), k=np.array([k_smooth, k_vertex], np.int64))


def main():
    ref = import_reference(sys.argv[1])
    verts, faces = neck_torus()
    out = dict(verts=verts, faces=faces, num_rays=np.int64(NUM_RAYS), seed=np.int64(SEED))
    for name, n, ks, kv in (("all", -1, K_SMOOTH[0], K_VERTEX[0]), ("sampled", SAMPLED, K_SMOOTH[1], K_VERTEX[1])):
        for k, v in run(ref, verts, faces, n, ks, kv).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sdf_ray_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
