"""GPU tests of the tile rasteriser at the list lengths where its list phase and its pass 3 change their path (``pytest -m gpu``):
the rows of 64 entries a binned list is read in, the longest list the list phase keeps on chip (512 entries; longer ones are read
from memory three times), the truncation switch (list longer than K), the 64-face groups of pass 3 (one of them without records
between two that have some) and the early exit of pass 1.  Behaviour only: every case is checked against the CPU oracle under the
kernel's own selection rule (``select_mode(1)``: the K nearest by (depth, face id)), two list lengths on either side of the on-chip
limit against each other bit for bit, and the fused launch against itself.

One 24 x 24 image (3 x 3 tiles), a stack of M triangles with their own vertices around one pixel centre of the centre tile, which
every face contains: that pixel has M candidates, so truncation starts exactly at M = K + 1.  The depths are a permutation of
1.5 + 0.002 i, so the order of the ids is not the order of the depths; every seventh face has a twin (same triangle, same depth, its
own vertices), so exact depth ties sit around the K-th place.  Three faces in four are about 3 px across and jittered by +-0.6 px;
every fourth is 6 to 8 px across and ends in an edge just inside of one pixel column, whose pixels lie outside of all those faces
within the blur reach: partially covered, and by more than K faces once M > 4 K - there the choice of the K nearest shows in the value."""
import functools

import numpy as np
import pytest
import torch

from oracle import render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 24
PX = 2.0 / S          # one pixel in NDC
CENTRE = 0.5 * PX     # the stack's centre: a pixel centre of the centre tile, inside every face of the stack
COPIES = 64           # images per fused launch: from 64 on the gradient is accumulated as packed fixed point


def _stack(M, gap=False):
    """(V, 3) vertices and (M, 3) faces of the stack.  ``gap``: faces 64 .. 127 keep one vertex inside the centre tile's box (0.1 px
    from its corner, 0.57 px from the nearest pixel centre: beyond the blur reach of 0.36 px) and have the other two 14 to 16 px
    away, outside the tile: the centre tile lists them and gets no candidate from them.  The library takes K <= 128, so a list of 192
    is always walked near to far, by the first radix digit of the faces' depths (64 buckets over the tile's depth range, each at
    most 1/32 of it wide): the three runs of 64 ids get depths 1.5, 1.6 and 1.7 + 0.0005 i, 0.068 apart where the range is 0.23, so
    no bucket holds faces of two runs and the moved faces are positions 64 .. 127 of the list - a whole group of pass 3."""
    rng = np.random.default_rng(4000 + M)
    depth = 1.5 + 0.002 * rng.permutation(M)
    if gap:
        depth = np.concatenate([1.5 + 0.1 * g + 0.0005 * rng.permutation(64) for g in range((M + 63) // 64)])[:M]
    v = np.zeros((M, 3, 3), np.float64)
    for i in range(M):
        if i % 7 == 1:  # the twin of face i - 1: an exact tie in every pixel, whatever the rounding of the interpolation
            v[i] = v[i - 1]
            continue
        if i % 4 == 0:  # 6 to 8 px across, with one edge 0.2 to 0.38 px inside of the pixel column 3 px right of the stack's centre
            xe = CENTRE + (3.0 - rng.uniform(0.2, 0.38)) * PX
            v[i, :, 0] = (xe, xe, CENTRE - rng.uniform(2.5, 3.5) * PX)
            v[i, :, 1] = (CENTRE - rng.uniform(2.2, 2.8) * PX, CENTRE + rng.uniform(2.2, 2.8) * PX, CENTRE + rng.uniform(-0.5, 0.5) * PX)
        else:           # about 3 px across, jittered by +-0.6 px: its inscribed circle (0.95 px) still holds the stack's centre
            ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
            c = CENTRE + rng.uniform(-0.6, 0.6, 2) * PX
            v[i, :, 0] = c[0] + 1.9 * PX * np.cos(ang)
            v[i, :, 1] = c[1] + 1.9 * PX * np.sin(ang)
        v[i, :, 2] = depth[i]
    if gap:
        corner = 1.0 / 3.0 - 0.1 * PX
        for i in range(64, min(128, M)):
            j = rng.uniform(-0.5, 0.5, 2) * PX
            v[i, 0, :2] = corner
            v[i, 1, :2] = (corner + 16 * PX + j[0], corner + 14 * PX)
            v[i, 2, :2] = (corner + 14 * PX, corner + 16 * PX + j[1])
            v[i, :, 2] = depth[i]
    faces = np.arange(3 * M, dtype=np.int32).reshape(M, 3)
    return v.reshape(3 * M, 3).astype(np.float32), faces


def _with_sliver(verts, faces):
    """One more face: a sliver 1.2 px long and 0.01 px thick along the border between two pixel rows (0.49 px from the nearest pixel
    centres: a candidate of no pixel), from the left neighbour tile into the centre tile's box, at a depth inside the stack's range.
    Shorter than the stack's large faces, so the image's bound on a vertex gradient - the fixed-point scale of a packed launch - stays."""
    z = 1.5 + 0.002 * 200.5
    sl = np.array([[-1.0 / 3.0 - 0.8 * PX, 0.0, z], [-1.0 / 3.0 + 0.4 * PX, 0.0, z], [-1.0 / 3.0 - 0.8 * PX, 0.01 * PX, z]], np.float32)
    V = verts.shape[0]
    return np.concatenate([verts, sl]), np.concatenate([faces, np.array([[V, V + 1, V + 2]], np.int32)])


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(11)
    gs = torch.randn(1, S, S, generator=g).numpy().astype(np.float32)
    target = (torch.rand(1, S, S, generator=g) > 0.5).float().numpy()
    return gs, target


@functools.lru_cache(maxsize=None)
def _reference(M, K, gap):
    """The oracle's silhouette, candidate counts and gradients for a case: computed once, shared, never written to."""
    verts, faces = _stack(M, gap)
    gs, target = _inputs()
    with render_ref.select_mode(1):
        sil, ncand = render_ref.silhouette_forward_np(verts[None], faces, S, K=K)
        want_b = render_ref.silhouette_backward_np(verts[None], faces, S, gs, K=K)[..., :2]
        g_fused = (np.sign(sil - target) / (S * S)).astype(np.float32)
        want_f = render_ref.silhouette_backward_np(verts[None], faces, S, g_fused, K=K)[..., :2]
    for a in (sil, ncand, want_b, want_f):
        a.setflags(write=False)
    return verts, faces, sil, ncand, want_b, want_f


def _model(faces, V):
    from smilify_amd.p3d_renderer import _MeshTopology

    return _MeshTopology(np.ascontiguousarray(faces), V, torch.device(DEV)).dm


def _fused(eng, dm, verts, K):
    _, target = _inputs()
    ndc = torch.from_numpy(verts)[None].repeat(COPIES, 1, 1).contiguous().to(DEV)
    tgt = torch.from_numpy(target).repeat(COPIES, 1, 1).contiguous().to(DEV)
    scale = torch.full((COPIES,), 1.0 / (S * S), device=DEV)
    return eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), scale, eng.raster_settings(K=K))


def _gradient_error(got, want):
    err = np.abs(got - want) / np.abs(want).max()
    return float(err.max()), float(np.sqrt((err ** 2).mean()))


# row and on-chip-limit boundaries, the truncation switch, pass-3 group boundaries, a group without records, the early exit
CASES = [(M, 100, False) for M in (1, 63, 64, 65, 100, 101, 128, 129, 192, 255, 256, 257, 511, 512, 513, 700)]
CASES += [(6, 6, False), (7, 6, False), (700, 6, False), (192, 100, True)]


@pytest.mark.parametrize("M,K,gap", CASES, ids=[f"M{m}-K{k}" + ("-gap" if g else "") for m, k, g in CASES])
def test_stack_against_the_oracle(M, K, gap):
    """Forward, backward and the fused launch (64 copies: packed gradient) against the oracle, with the bounds the existing tests
    use under this selection rule: silhouette 2e-5, gradient 1e-3 (max) and 2e-5 (rms) of the largest component, loss 2e-5."""
    from smilify_amd import engine as eng

    verts, faces, sil, ncand, want_b, want_f = _reference(M, K, gap)
    gs, target = _inputs()
    partial = int(((sil > 1e-3) & (sil < 1.0 - 1e-3)).sum())
    print(f"M {M} K {K}: partial pixels {partial}, truncated pixels {int((ncand > K).sum())}, most candidates {int(ncand.max())}")
    assert partial >= 5, partial
    if M > K:
        assert int((ncand > K).sum()) >= 1
    if gap:  # (the scene this case is about: the moved faces give the centre tile nothing, the runs before and behind them do)
        assert int(ncand[0, 8:16, 8:16].max()) == M - 64
    dm = _model(faces, verts.shape[0])
    rs = eng.raster_settings(K=K)
    ndc = torch.from_numpy(verts)[None].contiguous().to(DEV)

    got = eng.silhouette_forward(dm, ndc, S, rs).cpu().numpy()
    d = float(np.abs(got - sil).max())
    print(f"  forward max |diff| {d:.3g}")
    assert d < 2e-5, d

    gb = eng.silhouette_backward(dm, ndc, S, torch.from_numpy(gs).to(DEV), rs).cpu().numpy()
    emax, erms = _gradient_error(gb, want_b)
    print(f"  backward error max {emax:.3g} rms {erms:.3g}")
    assert np.abs(want_b).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)

    li, dn, _ = _fused(eng, dm, verts, K)
    loss_ref = float(np.abs(sil - target).sum())
    np.testing.assert_allclose(li.cpu().numpy(), np.full(COPIES, loss_ref, np.float32), rtol=2e-5)
    dn = dn.cpu().numpy()
    assert np.array_equal(dn, np.broadcast_to(dn[:1], dn.shape))  # 64 times the same image: the same bits
    emax, erms = _gradient_error(dn[:1], want_f)
    print(f"  fused error max {emax:.3g} rms {erms:.3g}")
    assert np.abs(want_f).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)


def test_on_chip_list_and_memory_list_give_the_same_bits():
    """512 entries in the centre tile's list is the longest the list phase keeps on chip; one more face that no pixel sees - a sliver
    between two pixel rows, listed by the centre tile - sends the same tile down the other path.  Every pixel of the image and the
    gradient rows of the 512 faces' vertices must come out bit for bit the same: the gradient sums of a packed launch are integers,
    and the fp64 sums of at most K logarithms of this size are exact."""
    from smilify_amd import engine as eng

    M, K = 512, 100
    verts, faces, sil, ncand, _, _ = _reference(M, K, False)
    verts2, faces2 = _with_sliver(verts, faces)
    with render_ref.select_mode(1):
        sil2, ncand2 = render_ref.silhouette_forward_np(verts2[None], faces2, S, K=K)
    assert np.array_equal(ncand, ncand2) and np.array_equal(sil, sil2)  # the sliver is a candidate nowhere
    assert int((ncand[0, 8:16, 8:16] > K).sum()) >= 1
    out = []
    for v, f in ((verts, faces), (verts2, faces2)):
        dm = _model(f, v.shape[0])
        fwd = eng.silhouette_forward(dm, torch.from_numpy(v)[None].contiguous().to(DEV), S, eng.raster_settings(K=K))
        li, dn, _ = _fused(eng, dm, v, K)
        out.append((fwd.cpu(), li.cpu(), dn.cpu()))
    (fwd_a, li_a, dn_a), (fwd_b, li_b, dn_b) = out
    assert torch.equal(fwd_a, fwd_b)                       # every pixel of every tile, the centre tile's included
    assert torch.equal(li_a, li_b)
    assert float(dn_a.abs().max()) > 0 and torch.equal(dn_a, dn_b[:, :3 * M])
    assert float(dn_b[:, 3 * M:].abs().max()) == 0.0


@pytest.mark.parametrize("M", [300, 600])
def test_fused_launch_is_bit_reproducible(M):
    from smilify_amd import engine as eng

    verts, faces = _stack(M)
    dm = _model(faces, verts.shape[0])
    li_a, dn_a, _ = _fused(eng, dm, verts, 100)
    li_b, dn_b, _ = _fused(eng, dm, verts, 100)
    assert float(dn_a.abs().max()) > 0
    assert torch.equal(dn_a, dn_b) and torch.equal(li_a, li_b)
