"""GPU tests of the tile rasteriser where its record sweeps end (``pytest -m gpu``).  The blend sweep, the refinement sweep of the
selection and pass 3 (once per 64-face group) read the record stream in buffers of four rows of 64 records, two buffers per turn;
the buffer that meets the end of the range is processed for the rows that hold a record only.  The scenes put the number of records
of one (sub-)tile and of its 64-face groups on the edges of that code.

One 64 x 64 image (8 x 8 tiles).  Everything but one face lies inside the box of tile (4, 4), pixels 32 .. 39, blur reach (0.97 px)
included, so that tile's list is the whole scene and, while no pixel can close, its record count is the number of (pixel, face)
candidates the oracle counts there.  The scene is the stack of test_gpu_raster_list_lengths.py - triangles about 3 px across with
their own vertices around one pixel centre, permuted depths, every seventh face a twin of the one before - plus "unit" faces: 0.04 px
across on a pixel centre, a candidate of that pixel alone, one record each.  One more stack face sits in tile (1, 1): the image has
partially covered pixels even when tile (4, 4) holds a single record.

Every case asserts
 1. forward, backward and the fused launch against the CPU oracle under the kernel's selection rule, with the bounds of
    test_gpu_raster_list_lengths.py (silhouette 2e-5, gradient 1e-3 max and 2e-5 rms of the largest component, loss 2e-5), after
    checking that test's preconditions - and the record counts the case is about - on the oracle alone;
 2. a fused launch of 64 copies (from 64 images on the gradient is summed as packed integers) gives the same bits in every copy:
    silhouette, loss and gradient.  A launch of 4 copies gives the same silhouette and loss bits in every copy; its gradient ends in
    float atomics - a launch with fewer tiles than workgroups deals every tile out in pieces of pixels, so a vertex receives several
    adds in an order that changes from run to run - and is held to the oracle's bounds of 1;
 3. the fused launch equals a forward launch plus a backward launch with the upstream gradient the fused kernel forms: bit for bit on
    the silhouette.  The backward entry point never packs (float atomics, every contribution rounded in its tile's fixed-point scale
    and not in the image's), so its gradient repeats neither the packed launch's bits nor its own from run to run: the two gradients
    are compared within the bounds of 1."""
import functools

import numpy as np
import pytest
import torch

from oracle import render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64
PX = 2.0 / S
TILE = slice(32, 40)   # pixels of tile (4, 4), both axes
PACKED, FLOAT = 64, 4  # images per fused launch: packed fixed point from 64 on, float atomics below
SELR_WAVE = 6 * 64     # longest compact stream the selection finishes in registers (SELR rows of 64)


def _ndc(i):
    """NDC coordinate of the centre of image column (or row) i: both axes are flipped."""
    return -1.0 + (2 * (S - 1 - i) + 1) / S


C = _ndc(35)  # the stack's centre: faces reach 3.5 px from it, pixels 32 .. 38


def _tri(cx, cy, radius, angle, z):
    ang = angle + np.array([0.0, 2.1, 4.2])
    return np.stack([cx + radius * np.cos(ang), cy + radius * np.sin(ang), np.full(3, z)], axis=1)


def _stack_face(rng, z, cx=C, cy=C):
    j = rng.uniform(-0.6, 0.6, 2) * PX
    return _tri(cx + j[0], cy + j[1], 1.9 * PX, rng.uniform(0, 2 * np.pi), z)


def _unit_face(ix, iy, z):
    """0.04 px across around the centre of pixel (ix, iy): no other pixel centre lies within the blur reach.  Moved 0.005 px towards
    the middle of one edge, so that edge is the closest one by a margin (on the centre itself the three edges are equally far, and
    which of them a rounding picks decides which vertices receive the gradient)."""
    return _tri(_ndc(ix) - 0.005 * PX * np.cos(1.35), _ndc(iy) - 0.005 * PX * np.sin(1.35), 0.02 * PX, 0.3, z)


def _mesh(tris):
    tris = list(tris) + [_stack_face(np.random.default_rng(77), 1.55, _ndc(11), _ndc(11))]  # the face in tile (1, 1)
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def _candidates(tris, K=100):
    """The oracle's candidate count per pixel for a list of triangles alone."""
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    with render_ref.select_mode(1):
        return render_ref.silhouette_forward_np(v[None], f, S, K=K)[1][0]


INTERIOR = [(x, y) for y in range(33, 39) for x in range(33, 39)]  # a unit face here is listed by tile (4, 4) alone


def _stack(M, rng, z0=1.5, dz=0.002):
    depth = z0 + dz * rng.permutation(M)
    tris = []
    for i in range(M):
        tris.append(tris[-1].copy() if i % 7 == 1 else _stack_face(rng, depth[i]))  # (a twin: an exact tie in every pixel)
    return tris


@functools.lru_cache(maxsize=None)
def _scene_records(T):
    """At most 64 faces (one group of pass 3, a list that cannot truncate under K = 100) with exactly T records in tile (4, 4):
    stack faces while they fit, unit faces for the rest."""
    rng = np.random.default_rng(9000 + T)
    tris, total = [], 0
    while len(tris) < 36:
        t = _stack_face(rng, 1.5 + 0.002 * len(tris))
        n = int(_candidates([t]).sum())
        if total + n > T:
            break
        tris.append(t)
        total += n
    for k in range(T - total):
        ix, iy = INTERIOR[k % len(INTERIOR)]
        tris.append(_unit_face(ix, iy, 1.6 + 0.001 * k))
    assert len(tris) <= 64, len(tris)
    return _mesh(tris) + (100, {"records": T})


@functools.lru_cache(maxsize=None)
def _scene_stack(M, K):
    return _mesh(_stack(M, np.random.default_rng(5000 + M))) + (K, {"list": M})


@functools.lru_cache(maxsize=None)
def _scene_closed_group():
    """192 faces in three runs of 64 by depth (1.5, 1.6, 1.7 + 0.0005 i: no bucket of the first radix digit holds two runs, so the
    runs are the three groups of pass 3).  Run 1 is a stack: its 64 faces all cover the stack's centre pixel.  Run 2 is 64 unit faces
    on that pixel: under K = 6 it is closed when their chunks are staged, so group 2 has no record.  Run 3 is 64 unit faces on pixel
    (38, 38), which the stack does not reach: group 3 has records again."""
    rng = np.random.default_rng(6000)
    run1 = _stack(64, rng, 1.5, 0.0005)
    run2 = [_unit_face(35, 35, 1.6 + 0.0005 * k) for k in rng.permutation(64)]
    run3 = [_unit_face(38, 38, 1.7 + 0.0005 * k) for k in rng.permutation(64)]
    c1, c2, c3 = _candidates(run1), _candidates(run2), _candidates(run3)
    assert c1[35, 35] == 64 and c1[38, 38] == 0
    assert c2.sum() == 64 and c2[35, 35] == 64 and c3.sum() == 64 and c3[38, 38] == 64
    return _mesh(run1 + run2 + run3) + (6, {"list": 192})


@functools.lru_cache(maxsize=None)
def _scene_split():
    """4097 faces in the list of tile (4, 4): the smallest list whose first estimate (a quarter of the 64 x list pairs exist) exceeds
    the record stream, so the tile runs as two sub-tiles of 32 pixels; chunks from 128 on keep their first record in memory."""
    rng = np.random.default_rng(7000)
    M, n_unit = 33, 4064
    depth = 1.5 + 0.00002 * rng.permutation(M + n_unit)
    tris = [_stack_face(rng, depth[i]) for i in range(M)]
    tris += [_unit_face(*INTERIOR[k % len(INTERIOR)], depth[M + k]) for k in range(n_unit)]
    return _mesh(tris) + (6, {"list": 4097})


def _bits_to_float(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


@functools.lru_cache(maxsize=None)
def _scene_compact(n_cmp, extra_far=0):
    """K = 6.  Three near stack faces, then `nf` copies of one triangle and `nt` unit faces on the stack's centre, all far ones inside
    one bucket of the first radix digit (the copies at one depth: exact ties, cut by face id; the unit faces 64 ulp behind them, never
    among the K nearest).  Every pixel the far triangle covers is truncated and chooses that bucket, so the compact stream of the tile
    is its candidates of the far faces: nf x (pixels of the triangle) + nt = n_cmp, + the triangle's pixels per `extra_far` face."""
    rng = np.random.default_rng(8000)
    near = [_stack_face(rng, 1.5 + 0.002 * i) for i in range(3)]
    zf_bits = 0x3FC00000 + 0xC0000 + 0x1555  # 1.59...: the middle of a bucket for every bucket width from 2^13 to 2^15 ulp
    zf, zt = _bits_to_float(zf_bits), _bits_to_float(zf_bits + 64)
    far_tri = _tri(C + 0.13 * PX, C + 0.07 * PX, 1.5 * PX, 0.4, zf)  # (off the pixel centre: no pixel is equally far from two edges)
    p0 = int(_candidates([far_tri]).sum())
    nf, nt = n_cmp // p0, n_cmp % p0
    far = [far_tri.copy() for _ in range(nf + extra_far)] + [_unit_face(35, 35, zt) for _ in range(nt)]
    assert nf + 3 > 6 and len(near) + len(far) <= 64
    all_c, far_c = _candidates(near + far), _candidates(far)
    assert int(far_c[all_c > 6].sum()) == n_cmp + extra_far * p0 and np.array_equal(all_c > 6, far_c > 0)
    return _mesh(near + far) + (6, {"compact": n_cmp + extra_far * p0})


# records of the tile and of its one group: the edges of a row and of a buffer, one case per number of rows modulo 8 (1, 2, ... 7, 0, 1)
RECORDS = (1, 63, 64, 65, 128, 192, 255, 256, 257, 320, 384, 448, 511, 512, 513)
assert {(t + 63) // 64 % 8 for t in RECORDS} == set(range(8))
CASES = {f"records{t}": functools.partial(_scene_records, t) for t in RECORDS}
CASES.update({
    "list90-K100": functools.partial(_scene_stack, 90, 100),    # two groups, no truncation
    "list70-K6": functools.partial(_scene_stack, 70, 6),        # two groups, the second one closes out
    "list140-K6": functools.partial(_scene_stack, 140, 6),      # three groups
    "list200-K6": functools.partial(_scene_stack, 200, 6),      # four groups
    "closed-group": _scene_closed_group,
    "split-4097": _scene_split,
    "compact384": functools.partial(_scene_compact, SELR_WAVE),            # finished in registers
    "compact385": functools.partial(_scene_compact, SELR_WAVE + 1),        # one refinement sweep through memory first
    "compact-tied": functools.partial(_scene_compact, SELR_WAVE, 1),       # more than SELR x 64 exact ties: through memory to the end
})


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(23)
    gs = torch.randn(1, S, S, generator=g).numpy().astype(np.float32)
    target = (torch.rand(1, S, S, generator=g) > 0.5).float().numpy()
    return gs, target


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's results for a case: computed once, shared, never written to."""
    verts, faces, K, about = CASES[name]()
    gs, target = _inputs()
    with render_ref.select_mode(1):
        sil, ncand = render_ref.silhouette_forward_np(verts[None], faces, S, K=K)
        want_b = render_ref.silhouette_backward_np(verts[None], faces, S, gs, K=K)[..., :2]
        g_fused = (np.sign(sil - target) / (S * S)).astype(np.float32)
        want_f = render_ref.silhouette_backward_np(verts[None], faces, S, g_fused, K=K)[..., :2]
    for a in (sil, ncand, want_b, want_f):
        a.setflags(write=False)
    return verts, faces, K, about, sil, ncand, want_b, want_f


def _gradient_error(got, want):
    err = np.abs(got - want) / np.abs(want).max()
    return float(err.max()), float(np.sqrt((err ** 2).mean()))


def _fused(eng, dm, verts, target, K, copies):
    ndc = torch.from_numpy(verts)[None].repeat(copies, 1, 1).contiguous().to(DEV)
    tgt = torch.from_numpy(target).repeat(copies, 1, 1).contiguous().to(DEV)
    scale = torch.full((copies,), 1.0 / (S * S), device=DEV)
    return eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), scale, eng.raster_settings(K=K), want_sil=True)


@pytest.mark.parametrize("name", list(CASES))
def test_sweep_tails(name):
    from smilify_amd import engine as eng
    from smilify_amd.p3d_renderer import _MeshTopology

    verts, faces, K, about, sil, ncand, want_b, want_f = _reference(name)
    gs, target = _inputs()
    # the preconditions of test_gpu_raster_list_lengths.py and what the case is about, on the oracle alone
    partial = int(((sil > 1e-3) & (sil < 1.0 - 1e-3)).sum())
    in_tile = int(ncand[0, TILE, TILE].sum())
    print(f"{name}: faces {faces.shape[0]}, K {K}, partial pixels {partial}, truncated pixels {int((ncand > K).sum())}, "
          f"candidates in tile (4, 4) {in_tile}, {about}")
    assert partial >= 5, partial
    other = ncand[0].copy()
    other[TILE, TILE] = 0
    assert other[16:, :].sum() == 0 and other[:, 16:].sum() == 0  # beside tile (4, 4) only the face in tile (1, 1) has candidates
    if "list" in about:
        assert faces.shape[0] - 1 == about["list"]
    if faces.shape[0] - 1 > K:
        assert int((ncand > K).sum()) >= 1
    if "records" in about:
        assert in_tile == about["records"] and faces.shape[0] - 1 <= min(K, 64)

    dm = _MeshTopology(np.ascontiguousarray(faces), verts.shape[0], torch.device(DEV)).dm
    rs = eng.raster_settings(K=K)
    ndc = torch.from_numpy(verts)[None].contiguous().to(DEV)

    fwd = eng.silhouette_forward(dm, ndc, S, rs)
    d = float(np.abs(fwd.cpu().numpy() - sil).max())
    print(f"  forward max |diff| {d:.3g}")
    assert d < 2e-5, d

    gb = eng.silhouette_backward(dm, ndc, S, torch.from_numpy(gs).to(DEV), rs).cpu().numpy()
    emax, erms = _gradient_error(gb, want_b)
    print(f"  backward error max {emax:.3g} rms {erms:.3g}")
    assert np.abs(want_b).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)

    loss_ref = float(np.abs(sil - target).sum())
    for copies in (PACKED, FLOAT):
        li, dn, sl = _fused(eng, dm, verts, target, K, copies)
        np.testing.assert_allclose(li.cpu().numpy(), np.full(copies, loss_ref, np.float32), rtol=2e-5)
        assert torch.equal(sl, sl[:1].expand_as(sl)) and torch.equal(li, li[:1].expand_as(li))
        assert torch.equal(sl[:1], fwd)  # the fused launch's silhouette is the forward launch's
        if copies == PACKED:
            assert torch.equal(dn, dn[:1].expand_as(dn))  # integer sums: 64 times the same image, the same bits
        for n in range(0, copies, copies - 1):
            emax, erms = _gradient_error(dn[n:n + 1].cpu().numpy(), want_f)
            print(f"  fused x{copies} image {n}: error max {emax:.3g} rms {erms:.3g}")
            assert np.abs(want_f).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)

    # (dn: the launch of 4 copies) forward + backward with the fused kernel's own upstream gradient
    g_up = torch.sign(fwd - torch.from_numpy(target).to(DEV)) * torch.full((1, 1, 1), 1.0 / (S * S), device=DEV)
    two = eng.silhouette_backward(dm, ndc, S, g_up.contiguous(), rs).cpu().numpy()
    emax, erms = _gradient_error(two, dn[:1].cpu().numpy())
    print(f"  forward + backward against fused: max {emax:.3g} rms {erms:.3g}")
    assert np.abs(two).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)
