"""Scenes on which the silhouette rasteriser is pinned per pixel to the float64 restatement (``tests/raster_ref64.py``), shared by
``tests/test_raster_ref64_cpu.py`` (float32 oracle against float64: the yardsticks) and ``tests/test_gpu_raster_float64.py`` (HIP kernels
against float64, at 4 x the yardstick).  Every scene is seeded and one image; DESIGN 4.2.1 has the rules.

Families:
 models   the three model meshes posed as in ``test_gpu_edge_cases._scene(t, 1, S, dist, seed)``; K from 1 to 100, most hit pixels truncate
 partial  the synthetic model on images of one tile and of sides that are no multiple of the 8-pixel tile
 stacks   the designed stacks of ``test_gpu_raster_list_lengths.py`` (truncation with exact twins at the K-th place, on-chip and
          in-memory lists, 64-face groups of pass 3) and two scenes of ``test_gpu_raster_sweep_tails.py`` with more than 384 records in one tile
 cuts     the posed synthetic mesh with vertices pulled through ``z_clip``: the front triangle of a face with two vertices behind
          the plane and the front quadrilateral of a face with one are both visible
 launch   the (129, 100) stack as the fused entry point sees it in a launch of 64 copies (packed fixed point) and of 4 (float atomics)
"""
import functools
import zlib

import numpy as np
import torch

import raster_ref64

# float32 oracle (select_mode(1)) against float64, per family: the largest measured value over the family's scenes, rounded up to two
# digits.  Silhouette: max |diff| on sure pixels.  Gradient: error relative to the image's largest float64 component, upstream
# gradient zero on unsure pixels, as max and as rms (on `cuts` the depth channel too, relative to its own largest component; on `stacks`
# and `launch` the fused entry point's upstream gradient too).  tests/test_raster_ref64_cpu.py asserts measured <= Y and measured >= Y / 4.
Y_SIL = {"models": 4.0e-6, "partial": 4.3e-6, "stacks": 5.5e-6, "cuts": 3.1e-6, "launch": 3.8e-6}
Y_GRAD_MAX = {"models": 8.6e-6, "partial": 9.3e-6, "stacks": 1.1e-5, "cuts": 4.6e-6, "launch": 5.0e-6}
Y_GRAD_RMS = {"models": 7.6e-7, "partial": 8.1e-7, "stacks": 2.5e-6, "cuts": 4.7e-7, "launch": 5.9e-7}
FACTOR = 4.0  # the project's margin over a float32 yardstick

UNSURE_CAP = 0.08            # unsure pixels / pixels with a candidate, per scene
MODELS_SURE_TRUNCATED = 15   # every scene of `models` keeps at least this many sure truncated pixels

# name -> (family, builder key, arguments, S, K); a model scene's arguments: model, camera distance, seed of the pose.  (The stick at
# S = 32 and the mouse at S = 24 use seed 34: with seed 31, 12 % and 10 % of their hit pixels are unsure, above the cap - rule 4, pixels
# next to a vertex of a face seen from far away.  A scene that misses a cap is replaced, the cap stays.)
SCENES = {
    "stick-S32-K100": ("models", "model", ("stick", 2.7, 34), 32, 100),
    "stick-S48-K10": ("models", "model", ("stick", 2.7, 31), 48, 10),
    "mouse-S24-K100": ("models", "model", ("mouse", 4.0, 34), 24, 100),
    "synthetic-S40-K3": ("models", "model", ("synthetic", 2.2, 31), 40, 3),
    "synthetic-S24-K1": ("models", "model", ("synthetic", 2.2, 31), 24, 1),
    "synthetic-S8": ("partial", "model", ("synthetic", 2.2, 31), 8, 100),
    "synthetic-S9": ("partial", "model", ("synthetic", 2.2, 31), 9, 100),
    "synthetic-S20": ("partial", "model", ("synthetic", 2.2, 31), 20, 100),
    "synthetic-S60": ("partial", "model", ("synthetic", 2.2, 31), 60, 100),
    "stack-M7-K6": ("stacks", "stack", (7, False), 24, 6),
    "stack-M101-K100": ("stacks", "stack", (101, False), 24, 100),
    "stack-M129-K100": ("stacks", "stack", (129, False), 24, 100),
    "stack-M513-K100": ("stacks", "stack", (513, False), 24, 100),
    "stack-M700-K6": ("stacks", "stack", (700, False), 24, 6),
    "stack-M192-gap-K100": ("stacks", "stack", (192, True), 24, 100),
    "tails-list200-K6": ("stacks", "tails", ("list200-K6",), 64, 6),
    "tails-records513": ("stacks", "tails", ("records513",), 64, 100),
    "cut-synthetic-S48": ("cuts", "cut", (), 48, 100),
    "launch-M129-K100": ("launch", "stack", (129, False), 24, 100),
}
FAMILIES = ("models", "partial", "stacks", "cuts", "launch")
LAUNCH_COPIES = (64, 4)  # from 64 images on the fused entry point packs its gradient as fixed point; 4: float atomics, tiles dealt out in pieces

CUT_PULLED = {5: 2e-4, 40: 1e-5, 77: 4e-4}  # test_gpu_raster_clip.py::test_depth_gradient_of_cut_edges: vertex -> depth nearer than z_clip
CUT_EXTRA = 41  # one more vertex pulled through the plane (to 3e-4), a neighbour of vertex 40: the two faces they share keep a front TRIANGLE


def names(*families):
    return [n for n, s in SCENES.items() if s[0] in families]


def family(name):
    return SCENES[name][0]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    _, kind, args, S, K = SCENES[name]
    if kind == "stack":
        from test_gpu_raster_list_lengths import _stack

        verts, faces = _stack(*args)
    elif kind == "tails":
        import test_gpu_raster_sweep_tails as tails

        verts, faces, k = tails.CASES[args[0]]()[:3]
        assert tails.S == S and k == K
    else:
        from conftest import MODEL_FILES
        from smilify_amd import model_io
        from test_gpu_edge_cases import _scene

        key = "synthetic" if kind == "cut" else args[0]
        t = model_io.synthetic_model() if key == "synthetic" else model_io.load_model(MODEL_FILES[key])
        if kind == "cut":
            ndc = _scene(t, 1, S, 2.5, 3).clone()
            for v, z in CUT_PULLED.items():
                ndc[0, v, 2] = z
            ndc[0, CUT_EXTRA, 2] = 3e-4
        else:
            ndc = _scene(t, 1, S, args[1], args[2])
        verts, faces = ndc[0].numpy(), t.faces
    verts = np.ascontiguousarray(verts, np.float32)
    faces = np.ascontiguousarray(faces, np.int32)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


def scene(name):
    """(verts (V, 3) float32, faces (F, 3) int32, S, K) of a scene: read only, shared."""
    return _mesh(name) + SCENES[name][3:]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of a scene: computed once, shared, never written to."""
    verts, faces, S, K = scene(name)
    return raster_ref64.render(verts, faces, S, K=K)


@functools.lru_cache(maxsize=None)
def upstream(name):
    """Seeded noise with |g| >= 0.25 (S, S) float32, exactly 0 on the reference's unsure pixels, and a binary target."""
    S = SCENES[name][3]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))  # (the scene's own: adding a scene changes no other's)
    g = torch.randn(S, S, generator=gen)
    g = (torch.sign(g) + (g == 0).float()) * (0.25 + g.abs())
    target = (torch.rand(S, S, generator=gen) > 0.5).float().numpy()
    g = g.numpy().astype(np.float32)
    g[reference(name).unsure] = 0.0
    g.setflags(write=False)
    target.setflags(write=False)
    return g, target


def fused_upstream(name, scale):
    """The upstream gradient of the fused L1 entry point, as that kernel forms it: ``scale * sign(float32(sil) - target)``."""
    _, target = upstream(name)
    return (scale * np.sign(reference(name).sil.astype(np.float32) - target)).astype(np.float32)


def gradient_errors(got, want):
    """Per-component error relative to the largest float64 component: (errors, max, rms)."""
    err = np.abs(np.asarray(got, np.float64) - want) / np.abs(want).max()
    return err, float(err.max()), float(np.sqrt((err ** 2).mean()))
