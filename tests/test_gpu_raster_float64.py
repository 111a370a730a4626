"""GPU tests of the silhouette rasteriser, per pixel and per vertex component, against the float64 restatement with its autograd
gradient (``pytest -m gpu``; ``tests/raster_ref64.py``, scenes and yardsticks in ``tests/raster_cases.py``, rules in DESIGN 4.2.1).

Bounds, none taken from the kernel: 4 x what the float32 oracle itself measures against float64 on the scene's family (``Y_SIL``,
``Y_GRAD_MAX``, ``Y_GRAD_RMS``; asserted from both sides in ``tests/test_raster_ref64_cpu.py``), plus, for a gradient component, the
derived accumulator term ``A``: half a unit of the kernel's fixed-point sums per kept record that reaches the component.  A pixel
whose discrete decisions are not sure in float32 (``Image.unsure``) is left out of the forward comparison and has its upstream
gradient set to exactly 0, in the array both sides receive; nothing is masked on the result.  Exact zeros where nothing may flow.
Every case prints its worst error over its bound and the number of sure, unsure and truncated pixels."""
import numpy as np
import pytest
import torch

import raster_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(name, tables):
    from smilify_amd import engine as eng

    _, kind, args, _, _ = rc.SCENES[name]
    verts, faces, _, _ = rc.scene(name)
    if kind in ("stack", "tails"):
        from smilify_amd.p3d_renderer import _MeshTopology

        return _MeshTopology(np.ascontiguousarray(faces), verts.shape[0], torch.device(DEV)).dm
    return eng.DeviceModel(tables("synthetic" if kind == "cut" else args[0]), DEV)


def _ndc(name, copies=1):
    return torch.from_numpy(np.array(rc.scene(name)[0]))[None].repeat(copies, 1, 1).contiguous().to(DEV)


def _counts(im):
    hit = im.count > 0
    return f"pixels: sure {int((hit & ~im.unsure).sum())} unsure {int((hit & im.unsure).sum())} truncated {int(im.trunc.sum())}"


def _check_forward(name, got, what="forward"):
    """Every sure pixel within 4 Y_SIL of float64; a pixel without a candidate in float64 exactly 0."""
    im = rc.reference(name)
    bound = rc.FACTOR * rc.Y_SIL[rc.family(name)]
    assert got.shape == im.sil.shape and float(np.abs(got[im.count == 0]).max(initial=0.0)) == 0.0
    err = np.where(im.unsure, 0.0, np.abs(got.astype(np.float64) - im.sil))
    y, x = np.unravel_index(np.argmax(err), err.shape)
    print(f"{name} {what}: worst error / bound {err.max() / bound:.3f} ({err.max():.3g} / {bound:.3g}); {_counts(im)}")
    assert err.max() <= bound, (name, what, (int(y), int(x)), float(got[y, x]), float(im.sil[y, x]), int(im.count[y, x]), bool(im.trunc[y, x]))


def _check_gradient(name, got, g, what, quantum=None):
    """Per vertex component: error relative to the largest float64 component at most 4 Y_GRAD_MAX + A, rms at most 4 Y_GRAD_RMS; a
    vertex with a float64 gradient of exactly zero that no kept record reaches exactly zero."""
    im = rc.reference(name)
    fam = rc.family(name)
    want = im.gradient(g)[0]
    scale = np.abs(want[:, :2]).max()
    assert scale > 0
    err, emax, erms = rc.gradient_errors(got, want[:, :2])
    A = im.accumulator_term(g, quantum) / scale
    bound = rc.FACTOR * rc.Y_GRAD_MAX[fam] + A
    ratio = err / bound
    v, c = np.unravel_index(np.argmax(ratio), ratio.shape)
    rms_bound = rc.FACTOR * rc.Y_GRAD_RMS[fam]
    print(f"{name} {what}: worst error / bound max {ratio.max():.3f} ({err[v, c]:.3g} / {bound[v, c]:.3g}, A at most {A.max():.3g}) "
          f"rms {erms / rms_bound:.3f} ({erms:.3g} / {rms_bound:.3g}); {_counts(im)}")
    idle = ~im.touched(g) & (want[:, :2] == 0).all(1)
    assert float(np.abs(got[idle]).max(initial=0.0)) == 0.0
    assert ratio.max() <= 1.0, (name, what, (int(v), int(c)), float(got[v, c]), float(want[v, c]), float(scale))
    assert erms <= rms_bound, (name, what, erms, rms_bound)
    return want


@pytest.mark.parametrize("name", rc.names("models", "partial", "stacks", "cuts"))
def test_forward_per_pixel_against_float64(name, tables):
    from smilify_amd import engine as eng

    _, _, S, K = rc.scene(name)
    got = eng.silhouette_forward(_model(name, tables), _ndc(name), S, eng.raster_settings(K=K))[0].cpu().numpy()
    _check_forward(name, got)


@pytest.mark.parametrize("name", rc.names("models", "partial", "stacks", "cuts"))
def test_backward_per_component_against_autograd(name, tables):
    """Upstream gradient: seeded noise with |g| >= 0.25, exactly 0 on unsure pixels; the same array goes to both sides.  On the cut
    scene the depth channel too (``ClipDepth``), relative to its own largest float64 component, with no accumulator term."""
    from smilify_amd import engine as eng

    verts, _, S, K = rc.scene(name)
    im = rc.reference(name)
    g, _ = rc.upstream(name)
    dm = _model(name, tables)
    cd = eng.ClipDepth(DEV, 1) if im.src.shape[0] else None
    got = eng.silhouette_backward(dm, _ndc(name), S, torch.from_numpy(np.array(g))[None].to(DEV), eng.raster_settings(K=K), clip_depth=cd)
    want = _check_gradient(name, got[0].cpu().numpy(), g, "backward")
    if rc.family(name) == "cuts":
        fam = "cuts"
        dz = cd.dense(verts.shape[0]).numpy()[0]
        assert np.abs(want[:, 2]).max() > 0
        err, emax, erms = rc.gradient_errors(dz, want[:, 2])
        print(f"{name} depth channel: worst error / bound max {emax / (rc.FACTOR * rc.Y_GRAD_MAX[fam]):.3f} ({emax:.3g}) "
              f"rms {erms / (rc.FACTOR * rc.Y_GRAD_RMS[fam]):.3f} ({erms:.3g})")
        assert float(np.abs(dz[want[:, 2] == 0]).max(initial=0.0)) == 0.0
        assert emax <= rc.FACTOR * rc.Y_GRAD_MAX[fam] and erms <= rc.FACTOR * rc.Y_GRAD_RMS[fam], (emax, erms, int(np.argmax(err)))
    else:
        assert cd is None and np.abs(want[:, 2]).max() == 0


FUSED = [(n, 1) for n in rc.names("stacks")] + [(n, c) for n in rc.names("launch") for c in rc.LAUNCH_COPIES]


@pytest.mark.parametrize("name,copies", FUSED, ids=[f"{n}-x{c}" for n, c in FUSED])
def test_fused_l1_against_float64(name, copies, tables):
    """The fused L1 entry point with a binary seeded target and scale 1 / S^2: the loss per image (the entry point returns it
    unscaled) to 4 Y_SIL x hit pixels, the silhouette under the forward bound, the gradient under the backward bound.  These scenes
    have no unsure pixel: the entry point forms its upstream gradient itself.  A launch of 64 copies packs its gradient as fixed point
    in the image's scale (returned with ``packed_out=True``: the accumulator term uses it) and every copy equals the first bit for
    bit; a launch of 4 copies ends in float atomics with its tiles dealt out in pieces, and is held to float64 copy by copy."""
    from smilify_amd import engine as eng

    _, _, S, K = rc.scene(name)
    im = rc.reference(name)
    assert not im.unsure.any()
    _, target = rc.upstream(name)
    dm = _model(name, tables)
    ndc = _ndc(name, copies)
    tgt = torch.from_numpy(np.array(target))[None].repeat(copies, 1, 1).contiguous().to(DEV)
    scale = 1.0 / (S * S)
    pix_scale = torch.full((copies,), scale, device=DEV)
    rs = eng.raster_settings(K=K)
    li, dn, sl = eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), pix_scale, rs, want_sil=True)
    quantum = None
    if copies >= 64:
        row_scale = eng.silhouette_l1_fused(dm, ndc, S, tgt, eng.image_abs_sum(tgt), pix_scale, rs, packed_out=True)[3].cpu().numpy()
        assert (row_scale > 0).all() and (row_scale == row_scale[0]).all()  # packed rows, one scale: the image's
        quantum = float(row_scale[0])
        assert torch.equal(dn, dn[:1].expand_as(dn)) and torch.equal(sl, sl[:1].expand_as(sl)) and torch.equal(li, li[:1].expand_as(li))
    li, dn, sl = li.cpu().numpy(), dn.cpu().numpy(), sl.cpu().numpy()
    hit = int((im.count > 0).sum())
    loss64 = float(np.abs(im.sil - target).sum())
    loss_bound = rc.FACTOR * rc.Y_SIL[rc.family(name)] * hit * scale
    gf = rc.fused_upstream(name, scale)
    for n in range(copies if copies < 64 else 1):
        what = f"fused x{copies} image {n}"
        lerr = abs(float(li[n]) - loss64) * scale
        print(f"{name} {what}: loss error / bound {lerr / loss_bound:.3f} ({lerr:.3g} / {loss_bound:.3g})")
        assert lerr <= loss_bound, (name, what, float(li[n]), loss64)
        _check_forward(name, sl[n], what + " silhouette")
        _check_gradient(name, dn[n], gf, what, quantum)
