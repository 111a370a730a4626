"""GPU tests of the rounded blur boxes (``pytest -m gpu``): the setup kernel enters a face into a corner tile of its tile box only
when that tile can hold a record of it, and ``stage_faces`` cuts a face's rectangle inside a tile to the rows and columns within
the blur DISC of its bounding box (``raster_reach.h``; the predicate itself is brute-forced in ``test_raster_rounded_boxes_cpu.py``).
The culled entries and the trimmed pixels hold no record, so nothing a pixel keeps may change: the scenes put faces where the square
and the disc differ, and where the shorter lists move a tile's depth range and the moment its pixels close.

Pattern and bounds of ``test_gpu_raster_sweep_tails.py``: forward, backward and the fused launch against the CPU oracle under the
kernel's selection rule (silhouette 2e-5, gradient 1e-3 max and 2e-5 rms of the largest component, loss 2e-5); a fused launch of 64
copies (packed integer sums) gives the same bits in every copy; the fused launch's silhouette is the forward launch's bit for bit
and its gradient is the backward launch's within the oracle's bounds.  Under both tie rules: no scene has two faces at one depth,
so ``reference_queue`` keeps what ``depth_face_id`` keeps.  The cut-face scene is held to the bounds of ``test_gpu_raster_clip.py``
(vertices at |xy| ~ 1e2 NDC units: fp32 cancellation in both implementations)."""
import functools

import numpy as np
import pytest
import torch

from oracle import render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 8
PACKED, FLOAT = 64, 4  # images per fused launch: packed fixed point from 64 on, float atomics below
REG_FACES = 6 * 1024   # raster_common.h: SETUP_REG_ROUNDS * SETUP_THREADS faces stay in the setup kernel's registers


def _reach(S):
    return float(np.sqrt(render_ref.BLUR_RADIUS)) * S / 2  # pixels


def _ndc(p, S):
    """NDC coordinate of the (continuous) output column or row p: pixel p has its centre at p; both axes are flipped."""
    return -1.0 + (2.0 * (S - 1 - np.asarray(p, np.float64)) + 1.0) / S


def _face(px, z, S):
    px = np.asarray(px, np.float64)
    return np.concatenate([_ndc(px, S), np.broadcast_to(np.asarray(z, np.float64), (3,))[:, None]], 1)


def _tri(c, radius, angle, z, S):
    a = angle + np.array([0.0, 2.1, 4.2])
    return _face(np.stack([c[0] + radius * np.cos(a), c[1] + radius * np.sin(a)], 1), z, S)


def _mesh(tris, S, anchor=(11.0, 11.0)):
    """The triangles plus one 3.8 px face around `anchor` (tile (1, 1)): every image has partially covered pixels."""
    tris = list(tris) + [_tri(anchor, 1.9, 0.7, 1.55, S)]
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def _candidates(tris, S, K=100):
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    with render_ref.select_mode(1):
        return render_ref.silhouette_forward_np(v[None], f, S, K=K)[1][0]


def _tile(n, tx, ty):
    return n[ty * TILE:ty * TILE + TILE, tx * TILE:tx * TILE + TILE]


def _scene_diagonal(S, hit):
    """A right-angled face with 0.3 px legs in the tile diagonally opposite tile T across an inner tile corner; P, its right-angle
    vertex and the corner of its bounding box, lies at 45 degrees from C, the pixel centre of T nearest that corner.  hit = False: P is
    0.3 px beyond the reach from C - the blurred SQUARE covers C (asserted), the disc does not: the oracle counts no candidate in T.
    hit = True: the mirror image across the corner, at the reach - 0.05 px: C is a candidate of the face."""
    a = S // 16
    reach = _reach(S)
    if not hit:
        C, s, d, T = np.array([TILE * a, TILE * a], np.float64), -1.0, reach + 0.3, (a, a)
    else:
        C, s, d, T = np.array([TILE * a - 1, TILE * a - 1], np.float64), 1.0, reach - 0.05, (a - 1, a - 1)
    P = C + s * d * np.sqrt(0.5)
    assert 0.5 < abs(P[0] - C[0]) < reach - 0.05  # P lies in the diagonal tile, and the square around the face reaches C
    tri = _face([P, P + [0.3 * s, 0.0], P + [0.0, 0.3 * s]], 1.5, S)
    n = _candidates([tri], S)
    assert n.sum() >= 1 and (int(_tile(n, *T).sum()) >= 1 if hit else int(_tile(n, *T).sum()) == 0), (S, hit, int(_tile(n, *T).sum()))
    return _mesh([tri], S) + (S, 100)


def _scene_span(S=64):
    """One face across 3 x 3 tiles and more: no corner tile of its box is empty, its rows and columns are trimmed at the box's corners."""
    tri = _tri((28.0, 28.0), 14.0, 0.4, 1.5, S)
    n = _candidates([tri], S)
    assert sum(int(_tile(n, tx, ty).any()) for tx in range(8) for ty in range(8)) >= 9
    return _mesh([tri], S, anchor=(52.0, 8.0)) + (S, 100)


def _scene_thin(S=256):
    """A 0.3 px wide sliver along a diagonal of 40 x 37 px: most tiles of its box hold none of it."""
    p, d = np.array([100.0, 100.0]), np.array([40.0, 37.0])
    w = 0.3 * np.array([-d[1], d[0]]) / np.hypot(*d)
    tri = _face([p, p + d, p + d + w], 1.5, S)
    n = _candidates([tri], S)
    box = n[96:144, 96:144].reshape(6, TILE, 6, TILE).any((1, 3))
    assert n.sum() >= 100 and box.sum() <= 20  # of the 36 tiles around it
    return _mesh([tri], S) + (S, 100)


def _scene_corner(S=64):
    """A face over the image corner (0, 0), and a sub-pixel face outside the opposite corner whose blurred square reaches the last
    pixel while its disc does not: that face has no candidate at all."""
    over = _tri((-1.0, -1.0), 5.0, 0.2, 1.5, S)
    d = (_reach(S) + 0.3) * np.sqrt(0.5)
    P = np.array([S - 1 + d, S - 1 + d])
    outside = _face([P, P + [0.3, 0.0], P + [0.0, 0.3]], 1.4, S)
    assert int(_candidates([over], S).sum()) >= 5 and int(_candidates([outside], S).sum()) == 0
    return _mesh([over, outside], S, anchor=(30.0, 30.0)) + (S, 100)


def _scene_stack(S=64, M=14, K=4):
    """Fourteen faces of about 3.8 px around the common corner of tiles (3, 3), (4, 3), (3, 4), (4, 4), permuted depths, K = 4: the
    pixels around the corner truncate and close while the four lists - each without the faces that only its square reached - are walked."""
    rng = np.random.default_rng(31)
    depth = 1.5 + 0.002 * rng.permutation(M)
    tris = [_tri(31.5 + rng.uniform(-1.5, 1.5, 2), 1.9, rng.uniform(0, 2 * np.pi), depth[i], S) for i in range(M)]
    n = _candidates(tris, S, K)
    assert int((n > K).sum()) >= 4 and all(int(_tile(n, tx, ty).sum()) > 0 for tx in (3, 4) for ty in (3, 4))
    return _mesh(tris, S) + (S, K)


def _scene_through_memory(S=64):
    """6 160 faces are seven rounds of the setup kernel: boxes and depths go through the tables, no tile is culled, the staging still trims."""
    import test_gpu_raster_setup_tables as st

    v, f = st._grid(56, 55)
    assert f.shape[0] > REG_FACES
    return st._place(v, 1, 60, extent=0.8)[0], f, S, 100


def _scene_tile_built(S=64, M=40):
    """Forty faces that each cover most of the image: 8 list entries per face are far too few, the tiles build their lists from the
    tile boxes - a superset of what the setup kernel counted."""
    rng = np.random.default_rng(5)
    v = np.zeros((M, 3, 3))
    for i in range(M):
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
        v[i, :, 0] = 0.85 * np.cos(ang) + rng.uniform(-0.1, 0.1)
        v[i, :, 1] = 0.85 * np.sin(ang) + rng.uniform(-0.1, 0.1)
        v[i, :, 2] = 1.5 + 0.01 * i + rng.uniform(0.0, 0.3, 3)
    verts = v.reshape(3 * M, 3).astype(np.float32)
    faces = np.arange(3 * M, dtype=np.int32).reshape(M, 3)
    xy = verts[:, :2][faces]
    tiles = np.prod(np.floor((xy.max(1) + 1) * S / 2 / TILE).clip(0, 7) - np.floor((xy.min(1) + 1) * S / 2 / TILE).clip(0, 7) + 1, axis=1)
    assert tiles.sum() > 2 * 8 * M  # unblurred boxes alone need twice the list space
    return verts, faces, S, 100


CASES = {
    "diagonal-miss-64": functools.partial(_scene_diagonal, 64, False),
    "diagonal-hit-64": functools.partial(_scene_diagonal, 64, True),
    "diagonal-miss-256": functools.partial(_scene_diagonal, 256, False),
    "diagonal-hit-256": functools.partial(_scene_diagonal, 256, True),
    "span-3x3": _scene_span,
    "thin-diagonal-256": _scene_thin,
    "image-corner": _scene_corner,
    "stack-K4-tile-corner": _scene_stack,
    "through-memory": _scene_through_memory,
    "tile-built-lists": _scene_tile_built,
}


@functools.lru_cache(maxsize=None)
def _inputs(S):
    g = torch.Generator().manual_seed(23 + S)
    gs = torch.randn(1, S, S, generator=g).numpy().astype(np.float32)
    target = (torch.rand(1, S, S, generator=g) > 0.5).float().numpy()
    return gs, target


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's results for a case: computed once, shared by the two tie rules, never written to."""
    verts, faces, S, K = CASES[name]()
    gs, target = _inputs(S)
    with render_ref.select_mode(1):
        sil, ncand = render_ref.silhouette_forward_np(verts[None], faces, S, K=K)
        want_b = render_ref.silhouette_backward_np(verts[None], faces, S, gs, K=K)[..., :2]
        g_fused = (np.sign(sil - target) / (S * S)).astype(np.float32)
        want_f = render_ref.silhouette_backward_np(verts[None], faces, S, g_fused, K=K)[..., :2]
    for a in (sil, ncand, want_b, want_f):
        a.setflags(write=False)
    return verts, faces, S, K, sil, ncand, want_b, want_f


def _gradient_error(got, want):
    err = np.abs(got - want) / np.abs(want).max()
    return float(err.max()), float(np.sqrt((err ** 2).mean()))


def _fused(eng, dm, verts, S, target, rs, copies):
    ndc = torch.from_numpy(verts)[None].repeat(copies, 1, 1).contiguous().to(DEV)
    tgt = torch.from_numpy(target).repeat(copies, 1, 1).contiguous().to(DEV)
    scale = torch.full((copies,), 1.0 / (S * S), device=DEV)
    return eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), scale, rs, want_sil=True)


@pytest.mark.parametrize("tie_rule", ["depth_face_id", "reference_queue"])
@pytest.mark.parametrize("name", list(CASES))
def test_rounded_boxes(name, tie_rule):
    from smilify_amd import engine as eng
    from smilify_amd.p3d_renderer import _MeshTopology

    verts, faces, S, K, sil, ncand, want_b, want_f = _reference(name)
    gs, target = _inputs(S)
    partial = int(((sil > 1e-3) & (sil < 1.0 - 1e-3)).sum())
    print(f"{name} / {tie_rule}: S {S}, faces {faces.shape[0]}, K {K}, partial pixels {partial}, truncated pixels {int((ncand > K).sum())}")
    assert partial >= 5, partial

    dm = _MeshTopology(np.ascontiguousarray(faces), verts.shape[0], torch.device(DEV)).dm
    rs = eng.raster_settings(K=K, tie_rule=tie_rule)
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
        li, dn, sl = _fused(eng, dm, verts, S, target, rs, copies)
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


@pytest.mark.parametrize("tie_rule", ["depth_face_id", "reference_queue"])
def test_cut_faces(tables, tie_rule):
    """Faces across ``z_clip``: their front parts are emitted by whichever thread cut them, go through the tables and are never culled;
    the staging trims them on their own bounding box.  The scene and the bounds of ``test_gpu_raster_clip.py``: silhouette mean
    2e-5 with at most 2e-3 of the pixels off by 1e-3, gradient 6e-3 of its largest component; 64 copies give the same silhouette and
    loss bits (images with cut faces accumulate their gradient in floats)."""
    from smilify_amd import engine as eng

    t = tables("synthetic")
    dm = eng.DeviceModel(t, DEV)
    S = 48
    g = torch.Generator().manual_seed(5)
    ndc = torch.empty(1, t.V, 3)
    ndc[..., :2] = 0.9 * (torch.rand(1, t.V, 2, generator=g) - 0.5)
    ndc[..., 2] = 0.8 + torch.rand(1, t.V, generator=g)
    idx = torch.randperm(t.V, generator=g)[:5]
    ndc[0, idx, 2] = torch.tensor([2e-4, 1e-5, 4e-4, 3e-4, 1e-4])  # nearer than z_clip = 5e-4, in front of the camera
    behind = (ndc[0, :, 2].numpy()[t.faces.astype(np.int64)] < 5e-4).sum(1)
    n_cut = int(((behind == 1) | (behind == 2)).sum())
    assert n_cut >= 4
    rs = eng.raster_settings(tie_rule=tie_rule)
    gs = torch.from_numpy(np.cos(0.3 * np.arange(S * S)).astype(np.float32).reshape(1, S, S))
    target = (torch.rand(1, S, S, generator=g) > 0.5).float()
    with render_ref.select_mode(1):
        ref, _ = render_ref.silhouette_forward_np(ndc.numpy(), t.faces, S)
        want = render_ref.silhouette_backward_np(ndc.numpy(), t.faces, S, gs.numpy())[..., :2]
    fwd = eng.silhouette_forward(dm, ndc.to(DEV), S, rs)
    assert eng.raster_stats(dm, 1)["straddling_faces"] == n_cut
    d = np.abs(fwd.cpu().numpy() - ref)
    print(f"cut faces / {tie_rule}: {n_cut} cut, forward mean |diff| {d.mean():.3g}, off by 1e-3: {np.mean(d > 1e-3):.3g}")
    assert ref.sum() > 50 and d.mean() < 2e-5 and np.mean(d > 1e-3) < 2e-3, (ref.sum(), d.mean(), np.mean(d > 1e-3), d.max())
    got = eng.silhouette_backward(dm, ndc.to(DEV), S, gs.to(DEV), rs).cpu().numpy()
    scale = np.abs(want).max()
    print(f"  backward max error {np.abs(got - want).max() / scale:.3g} of the largest component")
    assert scale > 0 and np.abs(got - want).max() < 6e-3 * scale, (np.abs(got - want).max(), scale)
    copies = ndc.repeat(PACKED, 1, 1).contiguous().to(DEV)
    tgt = target.repeat(PACKED, 1, 1).contiguous().to(DEV)
    li, dn, sl = eng.silhouette_l1_fused(dm, copies, S, tgt, eng.image_abs_sum(tgt), torch.full((PACKED,), 1.0 / (S * S), device=DEV), rs,
                                         want_sil=True)
    assert torch.equal(sl, sl[:1].expand_as(sl)) and torch.equal(li, li[:1].expand_as(li)) and torch.equal(sl[:1], fwd)
    # (the loss is a sum over the silhouette just checked: off by at most S^2 x the mean bound, plus 2e-5 relative as everywhere)
    loss_ref = float(np.abs(ref - target.numpy()).sum())
    assert abs(float(li[0]) - loss_ref) <= S * S * 2e-5 + 2e-5 * loss_ref, (float(li[0]), loss_ref)
    g_up = torch.sign(fwd - target.to(DEV)) / (S * S)
    two = eng.silhouette_backward(dm, ndc.to(DEV), S, g_up.contiguous(), rs).cpu().numpy()
    sc = np.abs(two).max()
    assert sc > 0 and np.abs(dn[:1].cpu().numpy() - two).max() < 6e-3 * sc and np.abs(dn[-1:].cpu().numpy() - two).max() < 6e-3 * sc
