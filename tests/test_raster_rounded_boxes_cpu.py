"""CPU test of the rounded blur box (``smilify_amd/csrc/raster_reach.h``): which corner tiles of a face's tile box ``k_raster_setup``
leaves out of the lists, and which rows and columns ``stage_faces`` cuts from a face's rectangle inside a tile.

``tests/raster_reach_main.cpp`` is compiled around the header by a plain host compiler and walks every face the way the two kernels
do.  Here every face is brute-forced in float64 against EVERY pixel centre of the image: a pixel that is inside the face, or whose
squared distance to it is below ``blur``, must have survived both the cull and the trim (and the trim alone: a tile that builds its
own list sees faces the setup kernel would have culled).  The faces: sub-pixel ones, faces several tiles wide, thin diagonals whose
bounding box is mostly empty, faces across the image's edges and corners, and sub-pixel faces whose bounding-box corner lies at the
reach -+ 1e-4 px (and further off on either side) from the nearest pixel centre of the diagonally neighbouring tile.  The generator
is chosen so that culls and trims do occur - asserted, so the test cannot pass on a predicate that never says no."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import render_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "smilify_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "raster_reach_main.cpp")
TILE = 8
BLUR = float(np.float32(render_ref.BLUR_RADIUS))                # what the kernels compare with
SQRT_BLUR = float(np.sqrt(np.float32(BLUR), dtype=np.float32))  # what they are handed for the boxes
DELTAS = (-1e-4, 1e-4, -1e-3, 1e-3, 0.02, 0.05, 0.5)            # px beyond the reach; from 0.02 on (> the 0.01 px of slack) the tile is culled


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("reach") / "raster_reach_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), MAIN])
    return str(exe)


def _tri(c, radius, angle):
    a = angle + np.array([0.0, 2.1, 4.2])
    return np.stack([c[0] + radius * np.cos(a), c[1] + radius * np.sin(a)], 1)


def _adversarial(S, reach):
    """Per inner tile corner (a sample of them), quadrant and delta: a right-angled face of 0.3 px legs whose right-angle vertex P - the
    corner of its bounding box - lies at reach + delta from C, the nearest pixel centre of the diagonally opposite tile.  Returns the
    faces (output pixel coordinates) and per face (C's column, C's row, delta)."""
    rng = np.random.default_rng(11 + S)
    faces, about = [], []
    corners = [(a, b) for a in range(1, S // TILE) for b in range(1, S // TILE)]
    for k in rng.permutation(len(corners))[:6]:
        a, b = corners[k]
        for qx in (0, 1):
            for qy in (0, 1):
                for delta in DELTAS:
                    th = np.deg2rad(rng.uniform(35.0, 55.0))
                    sx, sy = (-1.0 if qx == 0 else 1.0), (-1.0 if qy == 0 else 1.0)  # from C towards the face
                    C = np.array([TILE * a if qx == 0 else TILE * a - 1, TILE * b if qy == 0 else TILE * b - 1], np.float64)
                    P = C + (reach + delta) * np.array([sx * np.cos(th), sy * np.sin(th)])
                    faces.append(np.stack([P, P + [0.3 * sx, 0.0], P + [0.0, 0.3 * sy]]))
                    about.append((int(C[0]), int(C[1]), delta))
    return faces, about


def _faces(S):
    rng = np.random.default_rng(5 + S)
    reach = np.sqrt(BLUR) * S / 2
    out = []
    for _ in range(80):   # sub-pixel, anywhere including just outside the image
        out.append(_tri(rng.uniform(-6.0, S + 5.0, 2), rng.uniform(0.05, 0.45), rng.uniform(0, 2 * np.pi)))
    for _ in range(16):   # several tiles wide
        out.append(_tri(rng.uniform(0.0, S, 2), rng.uniform(8.0, 25.0), rng.uniform(0, 2 * np.pi)))
    for _ in range(30):   # thin diagonals
        p = rng.uniform(0.0, S, 2)
        d = rng.choice([-1.0, 1.0], 2) * rng.uniform(0.6, 1.0, 2) * rng.uniform(10.0, 50.0)
        w = rng.uniform(0.05, 0.5) * np.array([-d[1], d[0]]) / np.hypot(*d)
        out.append(np.stack([p, p + d, p + d + w]))
    for _ in range(30):   # across the image's edges and corners
        c = np.where(rng.random(2) < 0.5, rng.uniform(-5.0, 3.0, 2), rng.uniform(S - 4.0, S + 4.0, 2))
        if rng.random() < 0.5:
            c[rng.integers(2)] = rng.uniform(0.0, S)
        out.append(_tri(c, rng.uniform(0.3, 6.0), rng.uniform(0, 2 * np.pi)))
    n_general = len(out)
    adv, about = _adversarial(S, reach)
    px = np.asarray(out + adv, np.float64)                     # (n, 3, 2) output pixel coordinates: column xo, row yo
    ndc = (-1.0 + (2.0 * (S - 1 - px) + 1.0) / S).astype(np.float32)
    return ndc, n_general, about


def _candidates(ndc, S):
    """(n, S, S) bool in output order: the pixel centre is inside the face or nearer than sqrt(blur), all in float64."""
    c = -1.0 + (2.0 * (S - 1 - np.arange(S)) + 1.0) / S
    px, py = np.meshgrid(c, c)                                 # [yo, xo]
    p = np.stack([px, py], -1).reshape(1, -1, 2)
    v = ndc.astype(np.float64)
    out = np.empty((len(v), S * S), bool)
    for i0 in range(0, len(v), 8):
        t = v[i0:i0 + 8]
        d2 = np.full((len(t), S * S), np.inf)
        sign = []
        for a, b in ((0, 1), (1, 2), (2, 0)):
            A, E = t[:, a, None, :], (t[:, b] - t[:, a])[:, None, :]
            rel = p - A
            u = np.clip((rel * E).sum(-1) / (E * E).sum(-1), 0.0, 1.0)
            r = rel - u[..., None] * E
            d2 = np.minimum(d2, (r * r).sum(-1))
            sign.append(rel[..., 0] * E[..., 1] - rel[..., 1] * E[..., 0])
        inside = ((sign[0] > 0) & (sign[1] > 0) & (sign[2] > 0)) | ((sign[0] < 0) & (sign[1] < 0) & (sign[2] < 0))
        out[i0:i0 + 8] = inside | (d2 < BLUR)
    return out.reshape(len(v), S, S)


@pytest.mark.parametrize("S", [64, 256])
def test_no_candidate_is_culled_or_trimmed(program, tmp_path, S):
    ndc, n_general, about = _faces(S)
    src, dst = tmp_path / "faces.f32", tmp_path / "masks.u8"
    ndc[:, :, :2].reshape(-1).tofile(src)
    printed = subprocess.check_output([program, str(S), repr(SQRT_BLUR), str(src), str(dst)], text=True).split()
    counts = {printed[i]: int(printed[i + 1]) for i in range(0, len(printed), 2)}
    masks = np.fromfile(dst, np.uint8).reshape(len(ndc), S, S)
    cand = _candidates(ndc, S)
    box, kept, trimmed = (masks & 1) != 0, (masks & 2) != 0, (masks & 4) != 0
    print(f"S {S}: {len(ndc)} faces, {int(cand.sum())} candidates, {counts}, pixels: box {int(box.sum())}, after the trim {int(trimmed.sum())}, "
          f"after cull and trim {int(kept.sum())}")
    assert cand.sum() > 1000 and counts["slots"] == int(box.sum()) and counts["kept"] == int(kept.sum())
    assert not (kept & ~trimmed).any() and not (trimmed & ~box).any()
    lost = cand & ~kept
    assert not lost.any(), [(int(f), int(y), int(x)) for f, y, x in np.argwhere(lost)[:10]]
    # not vacuous: whole tiles are culled, rows and columns are trimmed, in the general faces alone as well
    # (a culled tile is one whose rectangle the trim empties as well: the cull removes the list entry, not further pixels)
    assert counts["culled"] > 0 and int(kept.sum()) < int(box.sum())
    per_tile = lambda m: m[:n_general].reshape(n_general, S // TILE, TILE, S // TILE, TILE).any((2, 4))  # noqa: E731
    emptied = per_tile(box) & ~per_tile(kept)       # (face, tile) pairs that leave the lists / stage to nothing
    shrunk = per_tile(kept) & (box[:n_general] & ~kept[:n_general]).reshape(n_general, S // TILE, TILE, S // TILE, TILE).any((2, 4))
    need = (1, 5) if S == 64 else (5, 20)           # (at 64^2 the reach is under a pixel: the square has little to lose)
    print(f"  general faces: {int(emptied.sum())} (face, tile) pairs emptied, {int(shrunk.sum())} shrunk")
    assert int(emptied.sum()) >= need[0] and int(shrunk.sum()) >= need[1], (int(emptied.sum()), int(shrunk.sum()))
    # the faces at the reach: C, the nearest centre of the diagonal tile, is a candidate just inside the reach and not just outside;
    # its tile keeps the face within the slack and loses it beyond
    for k, (cx, cy, delta) in enumerate(about):
        f = n_general + k
        assert bool(cand[f, cy, cx]) == (delta < 0), (S, k, delta)
        assert box[f, cy, cx] or delta > 0.05, (S, k, delta)  # the blurred SQUARE does reach C (at 35 .. 55 degrees: up to reach x 0.22 beyond)
        tile = (slice(cy // TILE * TILE, cy // TILE * TILE + TILE), slice(cx // TILE * TILE, cx // TILE * TILE + TILE))
        if delta >= 0.02:
            assert not kept[f][tile].any() and not cand[f][tile].any(), (S, k, delta)
        if abs(delta) <= 1e-3:
            assert kept[f, cy, cx], (S, k, delta)
