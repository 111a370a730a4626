"""GPU tests of the setup kernel's two ways from pass 1 to pass 2 and of the tile kernel's scratch at its grid sizes (``pytest -m gpu``).

The setup kernel keeps every face's tile box and nearest depth in registers between its passes when the mesh has at most
``REG_ROUNDS`` rounds of ``SETUP_THREADS`` faces, and stores the per-image tables (tile boxes, depth ranges, group boxes) only for a
reader: ``tie_rule="reference_queue"``, the colour path, image sizes that are never binned - and an image whose lists turn out not to
fit, which writes them late, from the registers.  Behaviour
only: against the CPU oracle under the kernel's own selection rule (``select_mode(1)``) at the bounds of
``test_gpu_raster_list_lengths.py`` (silhouette 2e-5, gradient 1e-3 max / 2e-5 rms of the largest component, loss 2e-5) and of
``test_gpu_raster_clip.py`` for cut faces, and launches against each other bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import render_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG_ROUNDS, SETUP_THREADS = 6, 1024  # raster_common.h: SETUP_REG_ROUNDS, SETUP_THREADS
TILE = 8
LIST_CAP_PER_FACE = 8                # raster_common.h: list entries an image may have per face (S <= 256)


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _place(v, n, seed, extent=0.6):
    """``n`` rigid placements of the vertices ``v`` in the rasteriser's input space: rotated, scaled to ``extent``, depth around 2.5."""
    rng = np.random.default_rng(seed)
    c = v - v.mean(0)
    c = c / np.abs(c).max()
    out = np.empty((n, v.shape[0], 3), np.float32)
    for i in range(n):
        p = c @ _rot(rng).T
        out[i, :, :2] = extent * p[:, :2] + rng.uniform(-0.25, 0.25, 2)
        out[i, :, 2] = 2.5 + 0.5 * p[:, 2]
    return out


def _topology(faces, V):
    from smilify_amd.p3d_renderer import _MeshTopology

    return _MeshTopology(np.ascontiguousarray(faces.astype(np.int32)), V, torch.device(DEV)).dm


def _workspace(eng, dm, N, S, tail=0):
    """A workspace of this test's own in place of the device's shared one: pattern-filled, ``tail`` bytes longer than the library asks for."""
    from smilify_amd import _lib

    need = int(_lib.load().smil_raster_workspace_bytes(dm.handle, N, S))
    ws = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    eng._SHARED_WS[dm._ws_key()] = ws
    return ws, need


def _fused(eng, dm, ndc, S, target, rs=None, **kw):
    tgt = target.to(DEV)
    scale = torch.full((ndc.shape[0],), 1.0 / (S * S), device=DEV)
    return eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), scale, rs, **kw)


def _targets(N, S, seed):
    return (torch.rand(N, S, S, generator=torch.Generator().manual_seed(seed)) > 0.5).float()


def _gradient_error(got, want):
    err = np.abs(got - want) / np.abs(want).max()
    return float(err.max()), float(np.sqrt((err ** 2).mean()))


def _check_against_oracle(eng, dm, verts, faces, S, seed, tag):
    """Forward, backward and the fused launch of ``verts`` (N, V, 3) against the oracle."""
    N = verts.shape[0]
    g = torch.Generator().manual_seed(seed)
    gs = torch.randn(N, S, S, generator=g).numpy().astype(np.float32)
    target = _targets(N, S, seed + 1)
    with render_ref.select_mode(1):
        sil, _ = render_ref.silhouette_forward_np(verts, faces, S)
        want_b = render_ref.silhouette_backward_np(verts, faces, S, gs)[..., :2]
        g_fused = (np.sign(sil - target.numpy()) / (S * S)).astype(np.float32)
        want_f = render_ref.silhouette_backward_np(verts, faces, S, g_fused)[..., :2]
    ndc = torch.from_numpy(verts).contiguous().to(DEV)
    got = eng.silhouette_forward(dm, ndc, S).cpu().numpy()
    d = float(np.abs(got - sil).max())
    print(f"{tag}: forward max |diff| {d:.3g} (covered {float(sil.sum()):.0f} px)")
    assert sil.sum() > 50 and d < 2e-5, d
    gb = eng.silhouette_backward(dm, ndc, S, torch.from_numpy(gs).to(DEV)).cpu().numpy()
    emax, erms = _gradient_error(gb, want_b)
    print(f"{tag}: backward error max {emax:.3g} rms {erms:.3g}")
    assert np.abs(want_b).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)
    li, dn, _ = _fused(eng, dm, ndc, S, target)
    np.testing.assert_allclose(li.cpu().numpy(), np.abs(sil - target.numpy()).sum((1, 2)), rtol=2e-5)
    emax, erms = _gradient_error(dn.cpu().numpy(), want_f)
    print(f"{tag}: fused error max {emax:.3g} rms {erms:.3g}")
    assert np.abs(want_f).max() > 0 and emax < 1e-3 and erms < 2e-5, (emax, erms)


def _list_entries(verts, faces, S):
    """(tile, face) pairs of one image, counted generously and stingily: the faces' blurred boxes grown / shrunk by a pixel."""
    xy = verts[:, :2][faces]                                           # (F, 3, 2)
    r = np.sqrt(render_ref.BLUR_RADIUS)
    out = []
    for slack in (1.0, -1.0):
        lo = ((xy.min(1) - r + 1.0) * S - 1.0) * 0.5 - slack
        hi = ((xy.max(1) + r + 1.0) * S - 1.0) * 0.5 + slack
        lo, hi = np.clip(np.ceil(lo), 0, S - 1), np.clip(np.floor(hi), 0, S - 1)
        t = np.maximum(hi // TILE - lo // TILE + 1, 0)
        out.append(int((t[:, 0] * t[:, 1]).sum()))
    return out  # [at most, at least]


def test_tables_of_an_earlier_call_are_never_read(tables):
    """The default mode leaves the tile boxes, depth ranges and group boxes of ITS scene unwritten; ``reference_queue`` reads them.  On
    one workspace: scene A in the default mode, then scene B under ``reference_queue`` - bit for bit what scene B gives on a workspace
    nobody has used.  STICK (six rounds: the register path), 64 images @64^2: the packed-gradient launch, whose sums are integers.
    The colour path cannot follow a silhouette call on the same workspace: it carves a workspace of its own
    (``smil_colour_workspace_bytes``, the engine's ``_COLOUR_WS``), whose setup always stores the tables."""
    from smilify_amd import engine as eng

    t = tables("stick")
    assert (t.F + 63) // 64 * 64 <= REG_ROUNDS * SETUP_THREADS
    dm = eng.DeviceModel(t, DEV)
    N, S = 64, 64
    a, b = _place(t.v_template, N, 21, extent=0.7), _place(t.v_template, N, 22, extent=0.45)
    # far enough apart that the faces' tile boxes differ: the oracle's silhouettes of the first images do (STICK is thin: a silhouette is 100 to 200 pixels)
    sa, _ = render_ref.silhouette_forward_np(a[:1], t.faces, S)
    sb, _ = render_ref.silhouette_forward_np(b[:1], t.faces, S)
    assert np.abs(sa - sb).sum() > 100 and sb.sum() > 50
    ca = ((a[0][:, :2][t.faces].mean(1) + 1.0) * S * 0.5 // TILE).astype(int)
    cb = ((b[0][:, :2][t.faces].mean(1) + 1.0) * S * 0.5 // TILE).astype(int)
    assert (ca != cb).any(1).mean() > 0.5  # most faces' centres lie in another tile
    target = _targets(N, S, 3)
    tie = eng.raster_settings(tie_rule="reference_queue")
    A, B = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    _workspace(eng, dm, N, S)
    _fused(eng, dm, A, S, target)
    got = [x.cpu() for x in _fused(eng, dm, B, S, target, tie, want_sil=True, packed_out=True)]
    _workspace(eng, dm, N, S)
    want = [x.cpu() for x in _fused(eng, dm, B, S, target, tie, want_sil=True, packed_out=True)]
    assert float(want[2].sum()) > 50 and bool(want[1].view(torch.int32).ne(0).any())  # (packed rows: integers, not floats)
    for name, g, w in zip(("loss_img", "d_ndc", "sil", "d_ndc_scale"), got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name  # (bits: a packed row read as floats holds NaNs)


def test_image_whose_lists_do_not_fit_writes_its_tables(tables):
    """Forty large faces that each cover most of the 64 tiles: 8 list entries per face are far too few, the image's tiles build their
    lists from the tables - which the setup kernel writes from its registers once the count shows that.  The same faces small in
    the second image of the launch: binned.  The decision is per image; both against the oracle, after a launch with the two images
    swapped, so that every table row of either image held something else before."""
    from smilify_amd import engine as eng

    S, M = 64, 40
    rng = np.random.default_rng(5)
    v = np.zeros((M, 3, 3))
    for i in range(M):
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
        v[i, :, 0] = 0.85 * np.cos(ang) + rng.uniform(-0.1, 0.1)
        v[i, :, 1] = 0.85 * np.sin(ang) + rng.uniform(-0.1, 0.1)
        v[i, :, 2] = 1.5 + 0.01 * i + rng.uniform(0.0, 0.3, 3)
    big = v.reshape(3 * M, 3)
    small = big.copy()
    small[:, :2] = 0.06 * big[:, :2] + 0.3
    faces = np.arange(3 * M, dtype=np.int32).reshape(M, 3)
    cap = LIST_CAP_PER_FACE * M
    assert _list_entries(big, faces, S)[1] > 2 * cap and _list_entries(small, faces, S)[0] <= 3 * cap // 4
    dm = _topology(faces, 3 * M)
    verts = np.stack([big, small]).astype(np.float32)
    eng.silhouette_forward(dm, torch.from_numpy(verts[::-1].copy()).to(DEV), S)
    _check_against_oracle(eng, dm, verts, faces, S, 40, "unbinned + binned")


@functools.lru_cache(maxsize=None)
def _grid(nx, ny):
    """A wavy sheet of nx x ny quads as 2 nx ny triangles, row by row."""
    gx, gy = np.meshgrid(np.linspace(-1, 1, nx + 1), np.linspace(-1, 1, ny + 1))
    v = np.stack([gx.ravel(), gy.ravel(), 0.25 * np.sin(3 * gx.ravel()) * np.cos(2 * gy.ravel())], 1)
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)], 1).reshape(-1, 3)
    return v, f.astype(np.int32)


@pytest.mark.parametrize("F", [REG_ROUNDS * SETUP_THREADS, REG_ROUNDS * SETUP_THREADS + 16],
                         ids=["rounds-at-the-bound", "one-round-more"])
def test_meshes_on_either_side_of_the_round_bound(F):
    """6 144 faces are exactly six rounds: boxes and depths stay in registers.  6 160 faces (a 56 x 55 grid) are seven: the tables go
    through memory as before.  The first mesh is the second cut short.  Two images @64^2 against the oracle."""
    from smilify_amd import engine as eng

    v, f = _grid(56, 55)
    assert f.shape[0] == REG_ROUNDS * SETUP_THREADS + 16
    f = f[:F]
    assert ((F + 63) // 64 * 64 <= REG_ROUNDS * SETUP_THREADS) == (F == REG_ROUNDS * SETUP_THREADS)
    verts = _place(v, 2, 60, extent=0.8)
    _check_against_oracle(eng, _topology(f, v.shape[0]), verts, f, 64, 61, f"F {F}")


def test_cut_faces_beside_the_register_path(tables):
    """Faces across ``z_clip`` in a launch that otherwise takes the register path: their front parts are emitted by whichever thread
    cut them and go through the tables.  One image against the oracle as ``test_gpu_raster_clip.py`` checks it; the counters of
    ``smil_raster_stats`` are what the CPU counts, and the same whether the tables are stored for all faces (``reference_queue``) or not."""
    from smilify_amd import engine as eng

    t = tables("synthetic")
    dm = eng.DeviceModel(t, DEV)
    S = 48
    g = torch.Generator().manual_seed(5)
    ndc = torch.empty(1, t.V, 3)
    ndc[..., :2] = 0.9 * (torch.rand(1, t.V, 2, generator=g) - 0.5)
    ndc[..., 2] = 0.8 + torch.rand(1, t.V, generator=g)
    # five vertices nearer than z_clip = 5e-4 but in front of the camera: the crossings stay inside the image (behind the camera the
    # front parts grow until they cover every pixel many times over, and an image that is opaque everywhere has no gradient to check)
    idx = torch.randperm(t.V, generator=g)[:5]
    ndc[0, idx, 2] = torch.tensor([2e-4, 1e-5, 4e-4, 3e-4, 1e-4])
    faces = t.faces
    behind = (ndc[0, :, 2].numpy()[faces.astype(np.int64)] < 5e-4).sum(1)
    n_cut = int(((behind == 1) | (behind == 2)).sum())
    assert n_cut >= 4 and int((behind == 1).sum()) >= 1 and int((behind == 2).sum()) >= 1  # quadrilaterals and triangles
    sil = eng.silhouette_forward(dm, ndc.to(DEV), S).cpu().numpy()
    st = eng.raster_stats(dm, 1)
    assert st["straddling_faces"] == n_cut and st["unclipped_faces"] == 0 and st["tiles"] > 0, st
    with render_ref.select_mode(1):
        ref, _ = render_ref.silhouette_forward_np(ndc.numpy(), faces, S)
    d = np.abs(sil - ref)
    assert ref.sum() > 50 and d.mean() < 2e-5 and np.mean(d > 1e-3) < 2e-3, (ref.sum(), d.mean(), np.mean(d > 1e-3), d.max())
    assert int(((sil > 0) | (ref > 0)).reshape(S // TILE, TILE, S // TILE, TILE).any((1, 3)).sum()) <= st["tiles"]
    gs = torch.from_numpy(np.cos(0.3 * np.arange(S * S)).astype(np.float32).reshape(1, S, S))
    got = eng.silhouette_backward(dm, ndc.to(DEV), S, gs.to(DEV)).cpu().numpy()
    with render_ref.select_mode(1):
        want = render_ref.silhouette_backward_np(ndc.numpy(), faces, S, gs.numpy())[..., :2]
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(got - want).max() < 6e-3 * scale, (np.abs(got - want).max(), scale)
    sil_q = eng.silhouette_forward(dm, ndc.to(DEV), S, eng.raster_settings(tie_rule="reference_queue")).cpu().numpy()
    st_q = eng.raster_stats(dm, 1)
    assert {k: st_q[k] for k in ("straddling_faces", "tiles", "unclipped_faces")} == {k: st[k] for k in ("straddling_faces", "tiles", "unclipped_faces")}
    assert np.abs(sil_q - ref).mean() < 2e-5


@pytest.mark.parametrize("N,S", [(1, 64), (64, 128)], ids=["smallest-grid", "largest-grid"])
def test_scratch_of_the_smallest_and_the_largest_grid(tables, N, S):
    """The tile kernel's per-workgroup scratch at the smallest grid the launch policy gives (one 64^2 image) and the largest (64
    images @128^2: every resident slot).  The fused call's silhouette is the forward call's, bit for bit; the fused call
    repeats itself bit for bit in the loss (integer sums) and, where the launch packs it, the gradient; and no byte behind what
    ``smil_raster_workspace_bytes`` asks for is touched."""
    from smilify_amd import engine as eng

    t = tables("stick")
    dm = eng.DeviceModel(t, DEV)
    ndc = torch.from_numpy(_place(t.v_template, N, 70 + N, extent=0.7)).to(DEV)
    target = _targets(N, S, 8)
    tail = 1 << 20
    ws, need = _workspace(eng, dm, N, S, tail=tail)
    fwd = eng.silhouette_forward(dm, ndc, S)
    first = _fused(eng, dm, ndc, S, target, want_sil=True, packed_out=True)
    again = _fused(eng, dm, ndc, S, target, want_sil=True, packed_out=True)
    assert dm._ws is ws                                              # (the calls did use this buffer)
    assert float(fwd.sum()) > 50 and torch.equal(first[2], fwd)
    assert torch.equal(first[0], again[0]) and torch.equal(first[3], again[3])
    packed = bool((first[3] != 0).any())
    assert packed == (N >= 64)
    if packed:
        assert bool(first[1].view(torch.int32).ne(0).any()) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))  # (packed rows: integers)
    else:  # float atomics: the order of arrival shows in the last bits
        sc = float(first[1].abs().max())
        assert sc > 0 and float((first[1] - again[1]).abs().max()) <= 1e-5 * sc
    assert bool((ws[need:] == 0xA5).all())
