"""The float64 restatement of the silhouette rasteriser (``tests/raster_ref64.py``) on the CPU: known answers of its own, its autograd
against central differences of its own forward, the float32 oracle against it on every scene of ``tests/raster_cases.py`` (the
yardsticks ``Y_SIL``, ``Y_GRAD_MAX``, ``Y_GRAD_RMS``, asserted from both sides) and the caps on what the sure / unsure rules may leave out."""
import functools
import math

import numpy as np
import pytest

import raster_cases as rc
import raster_ref64 as r64
from oracle import render_ref as rr

S = 32


def pix_ndc(i):  # output index -> NDC coordinate of the pixel centre (x: col, y: row)
    return 1.0 - (2 * i + 1) / S


def sigmoid(x):
    return 1 / (1 + math.exp(-x)) if x > -700 else 0.0


def _seg_d2(px, py, a, b):
    ba = b - a
    t = np.clip(np.dot(ba, np.array([px, py]) - a) / np.dot(ba, ba), 0, 1)
    q = a + t * ba
    return float((q[0] - px) ** 2 + (q[1] - py) ** 2)


def _tri_d2(px, py, tri):
    return min(_seg_d2(px, py, tri[0], tri[1]), _seg_d2(px, py, tri[0], tri[2]), _seg_d2(px, py, tri[1], tri[2]))


def _inside(px, py, tri):
    def e(a, b):
        return (px - a[0]) * (b[1] - a[1]) - (py - a[1]) * (b[0] - a[0])

    s = [e(tri[1], tri[2]), e(tri[2], tri[0]), e(tri[0], tri[1])]
    return all(x > 0 for x in s) or all(x < 0 for x in s)


# ----------------------------------------------------------------------------------------------------------------------------------
# known answers (the cases of tests/test_oracle_raster.py, restated for the restatement: float64 values, float64 bounds)
# ----------------------------------------------------------------------------------------------------------------------------------
def test_single_triangle_values_and_orientation():
    v = np.array([[0.1, 0.1, 2.0], [0.9, 0.1, 2.0], [0.1, 0.9, 2.0]], np.float32)  # +x, +y quadrant: top-left (NDC +x = left, +y = up)
    im = r64.render(v, np.array([[0, 1, 2]]), S)
    assert im.sil[: S // 2, : S // 2].sum() > 10 and im.sil[S // 2:, :].sum() == 0 and im.sil[:, S // 2:].sum() == 0
    assert im.count.max() == 1 and not im.trunc.any()
    tri = v[:, :2].astype(np.float64)
    lo, hi = float(v[0, 0]), float(v[1, 0])
    for yo in range(S):
        for xo in range(S):
            px, py = pix_ndc(xo), pix_ndc(yo)
            d = _tri_d2(px, py, tri)
            inside = px > lo and py > lo and (px - lo) + (py - lo) < hi - lo
            if not inside and d >= r64.BLUR:
                assert im.sil[yo, xo] == 0.0 and im.count[yo, xo] == 0
            else:
                want = sigmoid((d if inside else -d) / r64.SIGMA)
                assert abs(im.sil[yo, xo] - want) <= 1e-9 * max(want, 1e-30) + 1e-300, (yo, xo, im.sil[yo, xo], want)


def test_backface_rendered_and_behind_camera_skipped():
    front = np.array([[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [0.0, 0.5, 1.0]], np.float32)
    f = np.array([[0, 1, 2]])
    a = r64.render(front, f, S)
    b = r64.render(front[[0, 2, 1]].copy(), f, S)      # opposite winding
    assert a.sil.sum() > 10 and np.abs(a.sil - b.sil).max() < 1e-7  # (the area's + 1e-8 is the one term that sees the winding)
    behind = front.copy()
    behind[:, 2] = -1.0
    c = r64.render(behind, f, S)
    assert c.sil.sum() == 0 and c.count.sum() == 0
    # one vertex behind the camera: cut at z_clip, the front part (a quadrilateral: two triangles) is rendered
    strad = front.copy()
    strad[0, 2] = -0.1
    c = r64.render(strad, f, S)
    assert c.faces_aug.shape == (3, 3) and (c.faces_aug[0] == c.faces_aug[0][0]).all() and c.src.tolist() == [[0, 1], [0, 2]]
    va, fa, src, coef = rr.clip_faces_np(strad, f.astype(np.int32), 5e-4)
    assert np.array_equal(fa, c.faces_aug) and np.array_equal(src, c.src)
    np.testing.assert_allclose(c.clip_coef, coef, rtol=1e-12)
    assert c.sil.sum() > 10
    assert r64.render(strad, f, S, z_clip=0.0).sil.sum() == 0  # clipping off: the raw rule zmin < 1e-8 drops the face


def test_top_k_keeps_nearest_by_depth():
    K = 3
    big = [[-0.8, -0.8], [0.8, -0.8], [0.0, 0.8]]
    verts = np.array([[p[0], p[1], 1.0 + i] for i in range(6) for p in big], np.float32)
    f = np.arange(18).reshape(6, 3)
    c = S // 2
    for faces, want in ((f, [0, 1, 2]), (f[::-1].copy(), [5, 4, 3])):  # reversed submission order: the same three depths
        im = r64.render(verts, faces, S, K=K)
        assert im.count[c, c] == 6 and im.trunc[c, c] and not im.unsure[c, c]
        assert sorted(im.rec_face[im.rec_pixel == c * S + c].tolist()) == sorted(want)
    # equal depths at the K-th place: twins are cut by face id, and that is sure
    twins = np.concatenate([verts[:9], verts[6:9], verts[6:9]])
    im = r64.render(twins, np.arange(15).reshape(5, 3), S, K=K)
    assert sorted(im.rec_face[im.rec_pixel == c * S + c].tolist()) == [0, 1, 2] and not im.unsure[c, c]
    # a near-tie of faces that are no twins is not
    near = twins.copy()
    near[9:12, 2] = np.nextafter(np.float32(3.0), np.float32(4.0))
    near[9:12, 0] *= 0.99
    assert r64.render(near, np.arange(15).reshape(5, 3), S, K=K).unsure[c, c]


def test_alpha_product_over_faces():
    t1 = [[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [0.0, 0.5, 1.0]]
    t2 = [[-0.5, -0.52, 2.0], [0.5, -0.52, 2.0], [0.0, 0.5, 2.0]]
    v = np.array(t1 + t2, np.float32)
    im = r64.render(v, np.array([[0, 1, 2], [3, 4, 5]]), S)
    found = 0
    for yo in range(S):
        for xo in range(S):
            if im.count[yo, xo] == 2 and 0 < im.sil[yo, xo] < 0.999:
                px, py = pix_ndc(xo), pix_ndc(yo)
                p = []
                for tri in (v[:3, :2].astype(np.float64), v[3:, :2].astype(np.float64)):
                    d = _tri_d2(px, py, tri)
                    p.append(sigmoid((d if _inside(px, py, tri) else -d) / r64.SIGMA))
                want = 1 - (1 - p[0]) * (1 - p[1])
                assert abs(im.sil[yo, xo] - want) < 1e-12
                found += 1
    assert found > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# autograd against central differences of the restatement's own forward
# ----------------------------------------------------------------------------------------------------------------------------------
def _records(im):
    return sorted(zip(im.rec_pixel.tolist(), im.rec_face.tolist(), im.rec_a.tolist(), im.rec_b.tolist()))  # (a set: a depth step may reorder a pixel's records)


@pytest.mark.parametrize("name", ["stack-M101-K100", "cut-synthetic-S48"])
def test_autograd_against_central_differences(name):
    """The largest components of the gradient (x, y, and on the cut scene the depths of the cut edges' end points) against central
    differences with a step of 1e-7 (relative, for a depth): the forward is float64, so the difference quotient is good to ~1e-8 of
    the largest component.  A step that changes a discrete decision (candidate set, closest edge) says nothing and is left out."""
    verts, faces, S_, K = rc.scene(name)
    im = rc.reference(name)
    g, _ = rc.upstream(name)
    grad, gnew = im.gradient(g)
    loss = lambda r: float((r.sil * g.astype(np.float64)).sum())  # noqa: E731
    comps = [(int(i) // 2, int(i) % 2) for i in np.argsort(-np.abs(grad[:, :2]).reshape(-1))[:6]]
    if im.src.shape[0]:
        assert np.abs(grad[:, 2]).max() > 0
        comps += [(int(v), 2) for v in np.argsort(-np.abs(grad[:, 2]))[:6]]
        # render_ref.clip_depth_gradient, fed the new vertices' xy gradients, is what autograd gives through the crossing points
        dz = np.zeros(im.V)
        for j, (a, b) in enumerate(im.src):
            da, db = rr.clip_depth_gradient(verts[a].astype(np.float64), verts[b].astype(np.float64), gnew[j], r64.Z_CLIP)
            dz[a] += da
            dz[b] += db
        np.testing.assert_allclose(dz, grad[:, 2], rtol=1e-9, atol=1e-12 * np.abs(grad[:, 2]).max())
    else:
        assert np.abs(grad[:, 2]).max() == 0
    checked = 0
    for v, c in comps:
        scale = np.abs(grad[:, c if c == 2 else slice(0, 2)]).max()
        h = 1e-7 * (abs(float(verts[v, 2])) if c == 2 else 1.0)
        out = []
        for s in (+1, -1):
            x = verts.astype(np.float64)
            x[v, c] += s * h
            out.append(r64.render(x, faces, S_, K=K))
        if _records(out[0]) != _records(im) or _records(out[1]) != _records(im):
            continue
        fd = (loss(out[0]) - loss(out[1])) / (2 * h)
        assert abs(fd - grad[v, c]) <= 1e-6 * scale, (v, c, fd, grad[v, c])
        checked += 1
    assert checked >= len(comps) - 2, (checked, len(comps))


# ----------------------------------------------------------------------------------------------------------------------------------
# the float32 oracle against the restatement: yardsticks and caps
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _measure(name):
    verts, faces, S_, K = rc.scene(name)
    im = rc.reference(name)
    g, _ = rc.upstream(name)
    sure = ~im.unsure
    with rr.select_mode(1):
        sil, ncand = rr.silhouette_forward_np(verts[None], faces, S_, K=K)
        got = rr.silhouette_backward_np(verts[None], faces, S_, g[None], K=K)[0]
    sil0, _ = rr.silhouette_forward_np(verts[None], faces, S_, K=K)
    want, _ = im.gradient(g)
    out = {"sil": float(np.abs(sil[0] - im.sil)[sure].max()), "sil0_equal": bool(np.array_equal(sil0[0][~im.trunc], sil[0][~im.trunc])),
           "count_equal": bool(np.array_equal(ncand[0][sure], im.count[sure]))}
    _, out["gmax"], out["grms"] = rc.gradient_errors(got[:, :2], want[:, :2])
    if im.src.shape[0]:  # the depth channel of cut edges, relative to its own largest component
        _, zmax, zrms = rc.gradient_errors(got[:, 2], want[:, 2])
        out["gmax"], out["grms"] = max(out["gmax"], zmax), max(out["grms"], zrms)
    else:
        assert np.abs(want[:, 2]).max() == 0 and np.abs(got[:, 2]).max() == 0
    hit = im.count > 0
    out.update(hit=int(hit.sum()), unsure=int((im.unsure & hit).sum()), unsure_all=int(im.unsure.sum()), trunc=int(im.trunc.sum()),
               sure_trunc=int((im.trunc & sure).sum()))
    if rc.family(name) in ("stacks", "launch"):  # these scenes also go through the fused L1 entry point: its upstream gradient too
        gf = rc.fused_upstream(name, 1.0 / (S_ * S_))
        with rr.select_mode(1):
            got_f = rr.silhouette_backward_np(verts[None], faces, S_, gf[None], K=K)[0]
        _, fmax, frms = rc.gradient_errors(got_f[:, :2], im.gradient(gf)[0][:, :2])
        out["gmax"], out["grms"] = max(out["gmax"], fmax), max(out["grms"], frms)
    return out


def _round_up(x):
    """x rounded up to two significant digits."""
    e = math.floor(math.log10(x)) - 1
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_yardsticks_float32_oracle_against_float64(fam):
    """The constants of raster_cases.py are what the float32 oracle measures against float64, rounded up to two digits: asserted from
    both sides, so that a constant cannot go stale.  On pixels that do not truncate the faithful queue and the (depth, face id) rule
    give bit-equal float32 silhouettes, and on sure pixels oracle and restatement count the same candidates."""
    m = [_measure(n) for n in rc.names(fam)]
    for n, r in zip(rc.names(fam), m):
        print(f"{n}: sil {r['sil']:.3g} grad max {r['gmax']:.3g} rms {r['grms']:.3g}; hit {r['hit']} unsure {r['unsure']} truncated {r['trunc']}")
        assert r["sil0_equal"] and r["count_equal"], n
    for key, table in (("sil", rc.Y_SIL), ("gmax", rc.Y_GRAD_MAX), ("grms", rc.Y_GRAD_RMS)):
        worst = max(r[key] for r in m)
        print(f"{fam} {key}: measured {worst:.4g} -> {_round_up(worst):.2g}, written {table[fam]:.2g}")
        assert table[fam] / 4 <= worst <= table[fam], (fam, key, worst, table[fam])


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_caps_on_what_is_left_out(name):
    """Caps are conditions: a scene that misses one is replaced, never the cap."""
    r, im = _measure(name), rc.reference(name)
    fam = rc.family(name)
    assert r["hit"] > 0 and r["unsure"] <= rc.UNSURE_CAP * r["hit"], (r["unsure"], r["hit"])
    assert not (im.unsure & (im.count == 0)).any()  # (a pixel without a candidate is compared as exactly 0: it must be sure)
    if fam == "models":
        assert r["sure_trunc"] >= rc.MODELS_SURE_TRUNCATED, r["sure_trunc"]
    if fam in ("stacks", "launch"):  # the fused entry point cannot mask its upstream gradient
        assert r["unsure_all"] == 0
    g, _ = rc.upstream(name)
    assert np.array_equal(g == 0, im.unsure) and np.abs(g[~im.unsure]).min() >= 0.25


def test_families_keep_sure_truncated_pixels_and_the_cut_scene_shows_both_front_parts():
    for fams in (("models",), ("stacks", "launch")):
        for fam in fams:
            assert sum(_measure(n)["sure_trunc"] for n in rc.names(fam)) > 0, fam
    verts, faces, _, _ = rc.scene("cut-synthetic-S48")
    im = rc.reference("cut-synthetic-S48")
    nb = (verts[:, 2][faces] < r64.Z_CLIP).sum(1)
    F = faces.shape[0]
    parts, k = {}, F
    for fi in np.nonzero((nb == 1) | (nb == 2))[0]:  # front parts follow at F ... in the order of the cut faces: two for a quadrilateral
        n = 2 if nb[fi] == 1 else 1
        parts.update({k + j: n for j in range(n)})
        k += n
    assert k == im.faces_aug.shape[0]
    seen = {parts[f] for f in np.unique(im.rec_face[im.rec_face >= F])}
    assert seen == {1, 2}, seen  # a front triangle and a front quadrilateral are both candidates of pixels that keep them
