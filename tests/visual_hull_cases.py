"""TEST INFRASTRUCTURE ONLY: seeded scenes for the visual-hull tests - look-at rigs (``cameras.look_at_view_transform``) around an analytic
ellipsoid or a union of two, masks computed per PIXEL CENTRE in numpy float64 by intersecting the centre's ray with the ellipsoids (the
inverse of the projection ``visual_hull_ref.project`` restates, written separately here).

Grid origins and voxel sizes are deliberately incommensurate with the cameras: a grid centred on an optical axis puts whole columns of
voxel centres exactly on pixel edges, where the GPU's and numpy's float64 may legitimately disagree.  Condition (asserted for every case by
tests/test_visual_hull_cpu.py): at most ``AMBIGUOUS_CAP`` = 1e-4 of a case's voxels may touch an ambiguous (point, view) pair.

``get(name)`` builds a case once; ``reference(name)`` computes the restatement's carve of it once and shares it.
"""
import functools
from types import SimpleNamespace

import numpy as np

import visual_hull_ref as VR
from smilify_amd.cameras import look_at_view_transform

AMBIGUOUS_CAP = 1e-4
ELLIPSOID = (np.array([0.013, -0.021, 0.017]), np.array([0.45, 0.40, 0.52]))
SECOND = (np.array([0.2, 0.12, -0.15]), np.array([0.38, 0.40, 0.39]))
GRID_GX, GRID_GYZ = (1, 63, 64, 65), (1, 3, 5)


def rig(views, N=1, rows="views", radius=2.7, fov=30.0, aspect=False, principal=False, seed=0, azim0=11.3, elev=(-25.0, 35.0), fov_rows=1):
    """Camera dict of a ring looking at the origin.  rows: "one" (a single camera every view shares), "views" or "images" (N * views rows,
    every frame's ring its own); the aspect table holds ``views`` rows, the principal-point table N * views."""
    rng = np.random.default_rng(1000 + seed)
    n = {"one": 1, "views": views, "images": N * views}[rows]
    az = azim0 + (np.arange(n) % views) * (360.0 / views) + rng.uniform(-3.0, 3.0, n)
    R, T = look_at_view_transform(radius + rng.uniform(-0.1, 0.1, n), rng.uniform(elev[0], elev[1], n), az)
    cams = dict(R=R.numpy().astype(np.float32), T=T.numpy().astype(np.float32),
                fov=(fov + rng.uniform(-1.0, 1.0, fov_rows)).astype(np.float32))
    if aspect:
        cams["aspect_ratio"] = rng.uniform(0.9, 1.1, views).astype(np.float32)
    if principal:
        cams["principal_point"] = rng.uniform(-0.06, 0.06, (N * views, 2)).astype(np.float32)
    return cams


def ellipsoid_masks(cams, N, views, S, H, W, ellipsoids):
    """(N,views,H,W) bool: does the ray through the centre (r + 0.5, c + 0.5) of a pixel meet one of the ellipsoids (centre, radii) beyond
    the near plane.  float64 throughout."""
    R, T, k00, k11, pp = VR.camera_tables(cams, N, views)
    hS = 0.5 * S
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    out = np.zeros((N * views, H, W), bool)
    for n in range(N * views):
        Rinv = np.linalg.inv(R[n])
        yn, xn = (hS - ys) / hS - pp[n, 1], (hS - xs) / hS - pp[n, 0]
        d = np.stack([xn / k00[n], yn / k11[n], np.ones_like(xn)], axis=-1) @ Rinv  # X_view = X R + T  =>  X = (X_view - T) R^-1
        C = -T[n] @ Rinv
        for centre, radii in ellipsoids:
            p, q = (C - centre) / radii, d / radii
            a, b, c = (q * q).sum(-1), 2.0 * (q * p).sum(-1), (p * p).sum() - 1.0
            disc = b * b - 4.0 * a * c
            with np.errstate(invalid="ignore"):
                out[n] |= (disc >= 0.0) & ((-b + np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a) > VR.ZNEAR)  # (depth along d = z_view)
    return out.reshape(N, views, H, W)


def _case(name, *, N=1, views=2, S=64, H=64, W=64, grid=(8, 8, 8), voxel=0.05, origin=None, ellipsoids=(ELLIPSOID,), mask="u8", threshold=0.0,
          min_views=1, max_misses=0, outside_carves=False, empty_frame=None, clear_view=None, cams=None, **rig_args):
    c = SimpleNamespace(name=name, N=N, views=views, S=S, H=H, W=W, grid=tuple(grid), threshold=threshold, min_views=min_views,
                        max_misses=max_misses, outside_carves=outside_carves, ellipsoids=ellipsoids)
    c.cams = rig(views, N=N, **rig_args) if cams is None else cams
    c.voxel_size = np.asarray(voxel, np.float64).reshape(-1)
    if origin is None:  # around the world origin, off every axis by an irrational-looking amount
        origin = -0.5 * np.asarray(grid) * c.voxel_size[:, None] + np.array([0.0137, -0.0091, 0.0173])
    c.origin = np.asarray(origin, np.float64).reshape(-1, 3)
    fg = ellipsoid_masks(c.cams, N, views, S, H, W, ellipsoids)
    if empty_frame is not None:
        fg[empty_frame] = False
    if clear_view is not None:  # one view of every frame all background
        fg[:, clear_view] = False
    if mask == "u8":
        c.masks = (fg * 200).astype(np.uint8)
    elif mask == "bool":
        c.masks = fg
    else:  # float32 against a threshold, one foreground pixel of view 0 replaced by a NaN (background)
        c.masks = np.where(fg, 0.8, 0.3).astype(np.float32)
        r, col = np.argwhere(fg[0, 0])[len(np.argwhere(fg[0, 0])) // 2] if fg[0, 0].any() else (0, 0)
        c.masks[0, 0, r, col] = np.nan
    return c


def _grid_case(Gx, Gy, Gz):
    # three frames, the middle one's masks all background; two cameras near the +x and -x axes, 0.09 voxels: a 65-voxel row reaches
    # x = +-2.9, past both cameras - points behind a camera and outside the 48 x 80 masks
    return _case(f"grid_{Gx}_{Gy}_{Gz}", N=3, views=2, H=48, W=80, grid=(Gx, Gy, Gz), voxel=0.09, empty_frame=1, azim0=80.0, elev=(-10.0, 10.0),
                 seed=Gx + 7 * Gy + 31 * Gz)


BUILDERS = {
    # the analytic scenes of the first-principles tests (every view sees the whole ellipsoid)
    "ellipsoid32": lambda: _case("ellipsoid32", views=8, grid=(32, 32, 32), origin=(-0.8137, -0.7911, -0.8023), min_views=8, fov=27.0, elev=(-20.0, 30.0)),
    "two_ellipsoids": lambda: _case("two_ellipsoids", N=2, views=6, S=96, H=96, W=96, fov=36.0, grid=(28, 26, 24), voxel=0.062, ellipsoids=(ELLIPSOID, SECOND), min_views=6,
                                    rows="images", seed=3),
    # view counts
    **{f"views_{v}": (lambda v=v: _case(f"views_{v}", views=v, H=24, W=40, S=40, grid=(21, 6, 5), voxel=0.11, min_views=min(v, 2), seed=v))
       for v in (1, 2, 63, 64)},
    # camera tables of 1, views and N * views rows, with and without aspect_ratio and principal_point
    "rows_one": lambda: _case("rows_one", N=2, views=2, grid=(17, 9, 7), voxel=0.12, rows="one", seed=11),
    "rows_one_ap": lambda: _case("rows_one_ap", N=2, views=3, grid=(17, 9, 7), voxel=0.12, rows="one", aspect=True, principal=True, seed=12),
    "rows_views": lambda: _case("rows_views", N=2, views=3, grid=(17, 9, 7), voxel=0.12, rows="views", fov_rows=3, seed=13),
    "rows_views_ap": lambda: _case("rows_views_ap", N=2, views=3, grid=(17, 9, 7), voxel=0.12, rows="views", aspect=True, principal=True, seed=14),
    "rows_images": lambda: _case("rows_images", N=2, views=3, grid=(17, 9, 7), voxel=0.12, rows="images", fov_rows=6, seed=15),
    "rows_images_ap": lambda: _case("rows_images_ap", N=2, views=3, grid=(17, 9, 7), voxel=0.12, rows="images", aspect=True, principal=True,
                                    seed=16),
    # masks
    "mask_bool": lambda: _case("mask_bool", views=3, H=48, W=80, grid=(19, 11, 9), voxel=0.1, mask="bool", min_views=2, seed=21),
    "mask_f32_nan": lambda: _case("mask_f32_nan", views=3, H=48, W=80, grid=(19, 11, 9), voxel=0.1, mask="f32", threshold=0.5, min_views=2,
                                  seed=22),
    "mask_1x1": lambda: _case("mask_1x1", views=3, S=1, H=1, W=1, grid=(13, 11, 9), voxel=0.13, fov=20.0, clear_view=1, seed=23),
    # the vote rule: four views, grids that leave the images - voxels with every seen count 0 .. 4
    **{f"votes_m{m}": (lambda m=m: _case(f"votes_m{m}", views=4, H=48, W=80, grid=(33, 9, 7), voxel=0.1, min_views=3, max_misses=m, seed=31))
       for m in (0, 1)},
    # geometry: behind a camera and outside the image, outside_carves off and on
    **{f"outside_{int(o)}": (lambda o=o: _case(f"outside_{int(o)}", views=2, H=48, W=80, grid=(65, 5, 3), voxel=0.09, azim0=80.0,
                                               elev=(-10.0, 10.0), outside_carves=o, seed=41))
       for o in (False, True)},
    # voxel centres that float32 holds exactly (origin and voxel size dyadic): what query_points is asked at equals what the carve tests
    **{f"dyadic_{int(o)}": (lambda o=o: _case(f"dyadic_{int(o)}", N=2, views=3, H=48, W=80, grid=(33, 11, 9), voxel=0.09375,
                                              origin=(-1.59375, -0.46875, -0.40625), rows="images", aspect=True, principal=True, outside_carves=o,
                                              min_views=2, seed=61))
       for o in (False, True)},
    # per-frame origin and voxel size (with an empty frame in the middle), the anisotropic grid
    "per_frame": lambda: _case("per_frame", N=3, views=3, H=48, W=80, grid=(65, 3, 2), voxel=(0.05, 0.043, 0.061), empty_frame=1,
                               origin=[(-1.6137, -0.0791, -0.0523), (-1.4011, -0.0613, -0.0477), (-1.9873, -0.0991, -0.0571)], seed=51),
    **{f"grid_{gx}_{gy}_{gz}": (lambda gx=gx, gy=gy, gz=gz: _grid_case(gx, gy, gz)) for gx in GRID_GX for gy in GRID_GYZ for gz in GRID_GYZ},
}
# beyond 2^31 voxels in one call: two frames of 1.1e9 voxels, one view; checked at seeded voxel indices only (never built as a whole here)
BIG = dict(N=2, views=1, S=64, H=64, W=64, grid=(1100, 1000, 1000), voxel=0.0012, origin=(-0.6537, -0.5911, -1.0023), seed=71)


def big_case():
    """The BIG scene without a reference carve: masks and cameras only."""
    c = SimpleNamespace(name="big", threshold=0.0, min_views=1, max_misses=0, outside_carves=False, **{k: BIG[k] for k in ("N", "views", "S", "H", "W")})
    c.grid, c.voxel_size, c.origin = BIG["grid"], np.array([BIG["voxel"]]), np.array([BIG["origin"]])
    c.cams = rig(1, N=2, rows="images", seed=BIG["seed"], elev=(5.0, 25.0))
    c.masks = (ellipsoid_masks(c.cams, 2, 1, 64, 64, 64, (ELLIPSOID,)) * 255).astype(np.uint8)
    return c


GRID_CASES = [n for n in BUILDERS if n.startswith("grid_")]
SMALL_CASES = [n for n in BUILDERS if not n.startswith("grid_")]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(occ, votes) of ``visual_hull_ref.carve`` on the case.  Shared: leave it unchanged."""
    c = get(name)
    return VR.carve(c.masks, c.cams, c.S, c.origin, c.voxel_size, c.grid, c.min_views, c.max_misses, c.outside_carves, c.threshold)


def ambiguous_fraction(name):
    occ, v = reference(name)
    return 1.0 - float(v.exact.mean())


def scan_occupancy(N, grid, seed=0):
    """(N,Gz,Gy,Gx) uint8 built directly, for the scans of the per-workgroup counts (surface and mesh): frame 2 empty, every other frame six
    seeded balls of radius 2 to 5 voxels, and the first and the last voxel of the frame set - the counts of a frame's first and last
    workgroup are not zero, so a prefix that loses a round's carry shows in the very next frame."""
    Gx, Gy, Gz = grid
    rng = np.random.default_rng(4100 + seed)
    k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    occ = np.zeros((N, Gz, Gy, Gx), np.uint8)
    for n in range(N):
        if n == 2:
            continue
        for _ in range(6):
            c, r = rng.uniform(0.0, (Gx, Gy, Gz)), rng.uniform(2.0, 5.0)
            occ[n] |= ((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2 <= r * r).astype(np.uint8)
        occ[n, 0, 0, 0] = occ[n, -1, -1, -1] = 1
    return occ
