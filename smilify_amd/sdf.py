"""The per-vertex "spatial diameter" values that ``fit3d --use_sdf`` loads, computed on the HIP path: the reference's
``fitter_3d/SDF_tests.py`` (``compute_sdf``, ``smooth_distances``, ``assign_vertex_sdf``, ``process_obj_file``) and
``fitter_3d/SDF_batch.py`` (``process_mesh_folder``) with the same names and signatures, taking ``smilify_amd.mesh3d.Meshes`` where the
reference takes pytorch3d's.

* ``compute_sdf`` casts ``num_rays`` rays from every sample into the inward hemisphere and tests each against ALL faces in one HIP
  kernel (``csrc/raycast.hip``; the reference loops over samples and rays in Python, ~30 torch ops per ray).  A ray's value is the
  LARGEST hit distance, a sample's the mean of its rays' values inside (0.001, 0.2) bounding-box diagonals.
* ``smooth_distances`` / ``assign_vertex_sdf`` search their neighbours with the K-nearest kernel behind ``fit3d.knn_points`` (the
  reference: scipy's cKDTree), so 1 <= k <= 64 (``SMIL_KNN_MAX_K``) and k <= the number of points.

Two commands take a model and its scans to a registration with the term::

    python -m smilify_amd.sdf SCANS_DIR --output_dir OUT --model MODEL.npz
    python -m smilify_amd.fit3d --model MODEL.npz --mesh_dir SCANS_DIR --use_sdf --sdf_dir OUT/data

Deviations: a face with a zero normal raises ``ValueError`` (the reference returns NaN); a mesh that fails
raises instead of being skipped with a printed message; ``assign_vertex_sdf`` returns float32 (the reference float64, which
``fit3d.load_sdf_values`` casts to float32 anyway); neighbours at equal distance are ordered by index.  Not built, and raising where
reachable: the plots (``visualize_sdf``, ``visualize_vertex_sdf``), the debug ray view (``debug_single_vertex``, ``debug_mode``) and
the ``PerformanceMonitor``.  There is no acceleration structure: the exact maximum over all faces is the reference's value.
"""
from __future__ import annotations

import argparse
import glob
import os
import pickle
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib, engine
from . import config as _config
from .mesh3d import Meshes, load_obj

BATCH = 1000  # samples per batch of the reference's direction draws (SDF_tests.py:323)


def generate_random_directions_batch(normals: torch.Tensor, num_rays: int, device=None) -> torch.Tensor:
    """(B, num_rays, 3) unit directions in the hemisphere of ``-normals`` (B,3): randn, normalised, flipped where
    ``dir . (-normal) < 0`` (SDF_tests.py:225-250), drawn on the device of ``normals``."""
    d = torch.randn(len(normals), num_rays, 3, device=normals.device)
    d = d / torch.norm(d, dim=2, keepdim=True)
    dots = torch.bmm(d, -normals.unsqueeze(2)).squeeze(2)
    mask = dots < 0
    d[mask] = -d[mask]
    return d


def compute_sdf(mesh: Meshes, num_samples: int = 1000, num_rays: int = 30, directions: Optional[torch.Tensor] = None):
    """(sample_points (S,3), diameters (S,)) of a single mesh on a GPU (SDF_tests.py:253-384).

    ``num_samples`` -1 or F: every face once, sampled at its centroid.  Otherwise faces are drawn by ``torch.multinomial`` on their
    area and a point by ``w1 = sqrt(rand)``, ``w2 = rand (1 - w1)``, ``w0 = 1 - w1 - w2``.  Rays start at
    ``point + normal * 0.0001 diag`` and a sample's own face is never hit.  A ray is valid when its largest hit lies in
    ``(0.001 diag, 0.2 diag)``; a sample takes its first ``max(num_samples // 2, 1)`` valid rays (the reference's early exit) and
    their mean as float32, or ``0.001 diag`` without any.

    Every random number is drawn with the reference's torch ops on the CPU default generator, in the reference's order and in its
    batches of 1000 samples, and then uploaded: ``torch.manual_seed`` governs the result, and in all-faces mode a CPU run of the
    reference under the same seed sees the same directions.  ``directions`` (S, num_rays, 3) replaces the draw and is used as given
    (neither normalised nor flipped)."""
    dev = engine.require_gpu(mesh.device)
    if len(mesh) != 1:
        raise ValueError("compute_sdf: one mesh at a time")
    verts = mesh.verts_packed().detach().to(device="cpu", dtype=torch.float32)
    faces = mesh.faces_packed().detach().to(device="cpu", dtype=torch.int64)
    F = int(faces.shape[0])
    if F == 0 or (int(faces.min()) < 0 or int(faces.max()) >= int(verts.shape[0])):
        raise ValueError("compute_sdf: the mesh needs faces whose indices lie in [0, V)")
    num_rays = int(num_rays)
    if num_rays < 1:
        raise ValueError("compute_sdf: num_rays must be at least 1")
    diag = torch.norm(verts.max(dim=0)[0] - verts.min(dim=0)[0])
    d_lo, d_hi, offset = diag * 0.001, diag * 0.2, diag * 0.0001
    if num_samples == -1 or num_samples == F:  # (the reference draws F faces at random for num_samples = F and still takes centroids)
        num_samples = F
        face_idx = torch.arange(F)
    elif num_samples < 1:
        raise ValueError("compute_sdf: num_samples must be -1 or positive")
    else:
        fv = verts[faces]
        areas = 0.5 * torch.norm(torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1), dim=1)
        face_idx = torch.multinomial(areas / areas.sum(), num_samples, replacement=True)
    fv = verts[faces[face_idx]]
    if num_samples == F:
        points = torch.mean(fv, dim=1)
    else:
        w1 = torch.sqrt(torch.rand(num_samples))
        w2 = torch.rand(num_samples) * (1 - w1)
        w0 = 1 - w1 - w2
        points = w0.unsqueeze(-1) * fv[:, 0] + w1.unsqueeze(-1) * fv[:, 1] + w2.unsqueeze(-1) * fv[:, 2]
    normals = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)
    length = torch.norm(normals, dim=1, keepdim=True)
    # zero area is decided on the float64 cross product of the float32 edges, whose products are exact: a fused multiply-add may
    # leave a float32 cross product of parallel edges at a rounding residue instead of zero
    exact = torch.norm(torch.cross((fv[:, 1] - fv[:, 0]).double(), (fv[:, 2] - fv[:, 0]).double(), dim=1), dim=1)
    good = (exact > 0) & (length[:, 0] > 0) & torch.isfinite(length[:, 0])
    if not bool(good.all()):
        raise ValueError(f"compute_sdf: face {int(face_idx[int(torch.nonzero(~good)[0])])} has no normal (zero area or non-finite vertices)")
    normals = normals / length
    if directions is None:
        dirs = torch.cat([generate_random_directions_batch(normals[s:s + BATCH], num_rays) for s in range(0, num_samples, BATCH)])
    else:
        dirs = directions.detach().to(device="cpu", dtype=torch.float32)
        if tuple(dirs.shape) != (num_samples, num_rays, 3):
            raise ValueError(f"compute_sdf: directions of shape {tuple(dirs.shape)}, expected {(num_samples, num_rays, 3)}")
    origins = points + normals * offset
    cap = max(int(num_samples / 2), 1)
    diam, _ = engine.ray_diameters(verts.to(dev), faces.to(torch.int32).to(dev), origins.to(dev), face_idx.to(torch.int32).to(dev),
                                   dirs.to(dev), float(offset), float(d_lo), float(d_hi), cap)
    return points.to(dev), diam


def _knn(queries: torch.Tensor, points: torch.Tensor, k: int, what: str):
    from .fit3d import knn_points

    k, n = int(k), int(points.shape[0])
    if k < 1 or k > _lib.KNN_MAX_K:
        raise ValueError(f"{what}: k={k} outside 1 .. {_lib.KNN_MAX_K} (SMIL_KNN_MAX_K)")
    if k > n:
        raise ValueError(f"{what}: k={k} exceeds the {n} points")
    out = knn_points(queries.detach()[None], points.detach()[None], K=k)
    return out.dists[0], out.idx[0]


def smooth_distances(points: torch.Tensor, distances: torch.Tensor, k: int = 100):
    """(N,) the mean of ``distances`` over the k nearest of ``points`` (N,3), the point itself included (SDF_tests.py:387-415; the batch
    tool passes 50).  The mean is taken in float64 and rounded to the values' dtype."""
    engine.require_gpu(points.device)
    _, idx = _knn(points, points, k, "smooth_distances")
    return distances.detach().double()[idx].mean(dim=1).to(distances.dtype)


def assign_vertex_sdf(verts: torch.Tensor, sample_points: torch.Tensor, smoothed_diameters: torch.Tensor, k: int = 10) -> torch.Tensor:
    """(V,) float32 values of the vertices: the inverse-distance weighted mean (weights ``1 / (distance + 1e-6)``, normalised) of the
    values of the k nearest samples, min-max scaled to [0, 1], or zeros when constant (SDF_tests.py:775-818).  The weights and sums
    are float64, from the kernel's float32 squared distances."""
    engine.require_gpu(verts.device)
    d2, idx = _knn(verts, sample_points, k, "assign_vertex_sdf")
    w = 1.0 / (d2.double().sqrt() + 1e-6)
    w = w / w.sum(dim=1, keepdim=True)
    s = smoothed_diameters.detach().double()
    v = ((s - s.min())[idx] * w).sum(dim=1)  # (offsets from the smallest value: a constant field gives exact zeros)
    lo, hi = v.min(), v.max()
    v = (v - lo) / (hi - lo) if bool(hi > lo) else torch.zeros_like(v)
    return v.float()


def visualize_sdf(*_a, **_k):
    raise NotImplementedError("visualize_sdf: the plots are not part of the HIP path")


def visualize_vertex_sdf(*_a, **_k):
    raise NotImplementedError("visualize_vertex_sdf: the plots are not part of the HIP path")


def debug_single_vertex(*_a, **_k):
    raise NotImplementedError("debug_single_vertex: the debug ray view is not part of the HIP path")


def _values_of(verts: torch.Tensor, faces: torch.Tensor, num_samples: int, num_rays: int, k_smoothing: int, device):
    verts, faces = verts.to(device), faces.to(device)
    points, diam = compute_sdf(Meshes(verts=[verts], faces=[faces]), num_samples=num_samples, num_rays=num_rays)
    smoothed = smooth_distances(points, diam, k=k_smoothing)
    vertex_sdf = assign_vertex_sdf(verts, points, smoothed, k=10)
    return dict(sample_points=points.cpu(), smoothed_diameters=smoothed.cpu(), vertex_sdf=vertex_sdf.cpu(), verts=verts.cpu(),
                faces=faces.cpu())


def _save(result: dict, data_dir: str, name: str) -> str:
    """``NAME_sdf.pkl`` (the reference's record, CPU tensors) and ``NAME_sdf.npz`` (``vertex_sdf``; what fit3d.load_sdf_values
    prefers) in ``data_dir``."""
    os.makedirs(data_dir, exist_ok=True)
    path = os.path.join(data_dir, f"{name}_sdf.pkl")
    with open(path, "wb") as fh:
        pickle.dump(result, fh)
    np.savez(os.path.join(data_dir, f"{name}_sdf.npz"), vertex_sdf=result["vertex_sdf"].numpy().astype(np.float32))
    return path


def process_mesh_folder(input_dir: str, output_dir: str, num_samples: int = -1, num_rays: int = 30, k_smoothing: int = 50,
                        device="cuda") -> dict:
    """SDF_batch.py:23-147 without the plots: for every ``.obj`` under ``input_dir`` (recursively) ``data/NAME_sdf.pkl`` with the
    reference's keys and ``data/NAME_sdf.npz`` in ``output_dir``, and ``combined_sdf_results.pkl``.  Returns the combined record."""
    files = sorted(glob.glob(os.path.join(input_dir, "**/*.obj"), recursive=True))
    if not files:
        print(f"No .obj files found in {input_dir}")
        return {}
    data_dir = os.path.join(output_dir, "data")
    results = {}
    for mesh_file in files:
        name = Path(mesh_file).stem
        verts, faces = load_obj(mesh_file)
        r = _values_of(verts, faces, num_samples, num_rays, k_smoothing, device)
        r.update(mesh_file=mesh_file, num_vertices=len(r["verts"]), num_faces=len(r["faces"]), num_samples=num_samples, num_rays=num_rays,
                 k_smoothing=k_smoothing)
        results[name] = r
        print(f"Results saved to {_save(r, data_dir, name)}")
    with open(os.path.join(output_dir, "combined_sdf_results.pkl"), "wb") as fh:
        pickle.dump(results, fh)
    return results


def process_obj_file(obj_path: Optional[str] = None, output_dir: str = "sdf_output", num_samples: int = 1000, num_rays: int = 30,
                     debug_mode: bool = False, seed: int = 0, k_smoothing: int = 50, device="cuda") -> dict:
    """SDF_tests.py:870-980 without the plots: one OBJ file, or with ``obj_path`` None the template of
    ``smilify_amd.config.current.SMAL_FILE``, seeded with ``seed``; ``data/NAME_sdf.pkl`` and ``.npz`` in ``output_dir``."""
    if debug_mode:
        raise NotImplementedError("process_obj_file: the debug ray view is not part of the HIP path")
    torch.manual_seed(seed)
    np.random.seed(seed)
    if obj_path is None:
        if _config.current is None or _config.current.SMAL_FILE is None:
            raise ValueError("process_obj_file: no obj_path and smilify_amd.config.current names no SMAL_FILE")
        return process_model_file(_config.current.SMAL_FILE, output_dir, num_samples, num_rays, k_smoothing, seed=seed, device=device)
    verts, faces = load_obj(obj_path)
    r = _values_of(verts, faces, num_samples, num_rays, k_smoothing, device)
    r.update(num_samples=num_samples, num_rays=num_rays, seed=seed)
    print(f"Results saved to {_save(r, os.path.join(output_dir, 'data'), os.path.splitext(os.path.basename(obj_path))[0])}")
    return r


def process_model_file(model_path: str, output_dir: str, num_samples: int = -1, num_rays: int = 30, k_smoothing: int = 50,
                       seed: Optional[int] = None, device="cuda") -> dict:
    """The values of a SMIL model's ``v_template`` and faces, saved under the model file's stem: the name ``fit3d --use_sdf`` looks
    up for its source model."""
    from .model_io import load_model

    if seed is not None:
        torch.manual_seed(seed)
    t = load_model(model_path)
    r = _values_of(torch.from_numpy(np.asarray(t.v_template, np.float32)), torch.from_numpy(np.asarray(t.faces, np.int64)), num_samples,
                   num_rays, k_smoothing, device)
    r.update(mesh_file=model_path, num_samples=num_samples, num_rays=num_rays, k_smoothing=k_smoothing, seed=seed)
    print(f"Results saved to {_save(r, os.path.join(output_dir, 'data'), os.path.splitext(os.path.basename(model_path))[0])}")
    return r


def build_parser():
    p = argparse.ArgumentParser(description="Compute the spatial diameter values of every .obj in a folder (fitter_3d/SDF_batch.py on "
                                            "the HIP path)")
    p.add_argument("input_dir", type=str, help="Directory containing input OBJ files (searched recursively)")
    p.add_argument("--output_dir", type=str, default="sdf_batch_output", help="Directory to save the data (fit3d: --sdf_dir OUT/data)")
    p.add_argument("--num_samples", type=int, default=-1, help="Number of faces to sample. If -1, samples all faces (default: -1)")
    p.add_argument("--num_rays", type=int, default=30, help="Number of rays to cast per sampled point")
    p.add_argument("--k_smoothing", type=int, default=50, help="Number of neighbors for smoothing")
    p.add_argument("--seed", type=int, default=0, help="torch.manual_seed before the first mesh")
    p.add_argument("--model", type=str, default=None, help="also compute the values of this SMIL model's template (.pkl / .npz)")
    p.add_argument("--device", type=str, default="cuda")
    return p


def main(args) -> None:
    torch.manual_seed(args.seed)
    kw = dict(num_samples=args.num_samples, num_rays=args.num_rays, k_smoothing=args.k_smoothing, device=args.device)
    process_mesh_folder(args.input_dir, args.output_dir, **kw)
    if args.model is not None:
        process_model_file(args.model, args.output_dir, **kw)


if __name__ == "__main__":
    main(build_parser().parse_args())
