"""GPU tests of the LBS kernels (smilify_amd/csrc/lbs.hip) and the camera projection (project.hip) against FLOAT64 references
(tests/lbs_ref64.py: the CPU oracle evaluated in double; reference smal_model/smal_torch.py:198-370, batch_lbs.py:31-197,
p3d_renderer.py:112-137) at the sizes, options and poses where the kernels change form (``pytest -m gpu``).

Every forward output and every gradient is measured with ``row_err`` (per frame for per-frame quantities, so that a frame or a
table with a small gradient cannot hide behind a large one; a row that is exactly zero in the reference must be exactly zero)
against ``lbs_ref64.TOL``: 16 x the error the fp32 CPU oracle itself shows against float64 on the same cases
(tests/test_lbs_ref64_cpu.py keeps that measurement), never looser than the older tests' 2e-5 / 3e-4.  Each figure is printed
before it is asserted."""
import pytest
import torch

import lbs_ref64 as r64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
_SPECS = r64.lbs_specs(_CUS)
_ids = lambda v: v if isinstance(v, str) else ""  # noqa: E731


def _eng():
    from smilify_amd import engine

    return engine


@pytest.fixture(scope="module")
def dmodel(tables):
    cache = {}

    def get(key):
        if key not in cache:
            t = r64.get_tables(key, tables)
            cache[key] = (t, _eng().DeviceModel(t, DEV))
        return cache[key]

    return get


def _cams(up):
    return _eng().CameraSet(up["R"].to(DEV), up["T"].to(DEV), up["fov"].to(DEV), None, up["views"], up["S"])


def _run(dm, case, fused=False, repeat=False, **bwd_kw):
    """One call through the kernels: (forward outputs, gradients[, gradients of a second identical backward call])."""
    eng = _eng()
    B, inp, fl, up = case["B"], case["inp"], case["fl"], case["up"]
    cu = lambda d, k: None if d.get(k) is None else d[k].to(DEV).contiguous()  # noqa: E731
    kw = dict(trans=cu(inp, "trans"), logscale=cu(inp, "ls"), btrans=cu(inp, "bt"), del_v=cu(inp, "del_v"), v_template=cu(inp, "v_template"),
              Rs_in=cu(inp, "Rs_in"), theta_mask=cu(inp, "theta_mask"), **fl)
    beta, theta = cu(inp, "beta"), cu(inp, "theta")
    if up["views"]:
        cams, N = _cams(up), B * up["views"]
        d_ndc, d_yx = cu(up, "d_ndc"), cu(up, "d_yx")
        if fused:
            out = eng.lbs_forward(dm, beta, theta, project=dict(cams=cams, ndc=True, yx=True), **kw)
        else:
            out = eng.lbs_forward(dm, beta, theta, **kw)
            out["ndc"], out["yx"] = eng.project_verts_and_joints(cams, out["verts"], out["joints"])

        def backward():
            fov_img = torch.zeros(N, device=DEV)
            if fused:
                g = eng.lbs_backward(dm, out, None, None, ndc_upstream=dict(cams=cams, d_ndc=d_ndc, d_yx=d_yx, d_fov_img=fov_img), **bwd_kw)
            else:
                dv, dj = eng.project_backward_verts_and_joints(cams, out["verts"], d_ndc, out["joints"], d_yx, fov_img)
                g = eng.lbs_backward(dm, out, dv, dj, **bwd_kw)
                g["d_joints"] = dj
            g["d_fov"] = eng.fov_reduce(cams, fov_img)
            return g
    else:
        out = eng.lbs_forward(dm, beta, theta, **kw)

        def backward():
            return eng.lbs_backward(dm, out, cu(up, "d_verts"), cu(up, "d_joints"), need_vshaped="del_v" in inp or "v_template" in inp,
                                    need_Rs="Rs_in" in inp, up_Rs=cu(up, "up_Rs"), up_v_shaped=cu(up, "up_vs"), **bwd_kw)
    g = backward()
    if "v_template" in inp:  # (a custom template is one table shared by the batch: SMAL sums the per-frame gradient)
        g["d_v_template"] = g["d_del_v"].double().sum(0)
        if "del_v" not in inp:
            g["d_del_v"] = None
    fwd = dict(verts=out["verts"], joints=out["joints"], Rs=out["Rs"], A=out["A"].reshape(B, dm.J, 3, 4), new_J=out["new_J"], v_shaped=out["v_shaped"])
    if up["views"]:
        fwd.update(ndc=out["ndc"][..., :2], ndc_z=out["ndc"][..., 2], yx=out["yx"])
    g2 = backward() if repeat else None
    torch.cuda.synchronize()
    return (fwd, g, g2) if repeat else (fwd, g)


def _errors(what, fwd, grads, ref_f, ref_g, case):
    """row_err of everything the reference has, printed; returns the list of (what, quantity, error, bound) beyond the bound."""
    bad = []
    for k, want in list(ref_f.items()) + list(ref_g.items()):
        got = fwd[k] if k in ref_f else grads.get(k)
        if got is None:  # (no buffer came back: the reference must not depend on that input at all)
            err = 0.0 if not bool(want.any()) else float("inf")
        else:
            err = r64.row_err(got, want, r64.rows_of(k, case))
        print(f"{what:40s} {k:13s} {err:.3e}  (bound {r64.TOL[k]:.1e})")
        if not err <= r64.TOL[k]:
            bad.append((what, k, err, r64.TOL[k]))
    return bad


def _routes(eng, dm, case):
    """The routes a case takes: the separate kernels always; the fused per-frame kernels where the objective sits on the image
    plane and the library holds the model."""
    if case["up"]["views"] and eng.lbs_backward_ndc_supported(dm, case["nB_used"], case["up"]["views"]):
        return (("fused", True), ("separate", False))
    return (("separate", False),)


@pytest.mark.parametrize("cid,key,kw", _SPECS["batch"], ids=_ids)
def test_lbs_at_every_batch_size_where_the_kernels_change_form(cid, key, kw, dmodel):
    """B at few_frames (64), B <= CUs (the 1024-thread forms), SMALL_BATCH_FRAMES (256; ragged last blocks of 1 and 3 live
    waves at 257 and 259), and past grid = CUs x blocks per CU (blocks loop over frames); STICK with shared betas / tables and
    with per-frame betas, the mouse (static joints, one workgroup per CU).  Both routes against ONE float64 reference, and two
    backward calls return the same bits in the shared sums (BetaSum, smil_reduce_rows add their rows in a fixed order)."""
    eng = _eng()
    t, dm = dmodel(key)
    case = r64.build_case(t, kw)
    ref_f, ref_g = r64.reference(t, case)
    routes = _routes(eng, dm, case)
    assert len(routes) == 2, "STICK and the mouse take the fused kernels at every camera rig"
    bad = []
    for name, fused in routes:
        fwd, g, g2 = _run(dm, case, fused, repeat=True)
        bad += _errors(f"{cid}/{name}", fwd, g, ref_f, ref_g, case)
        for k in ("d_beta", "d_logscale", "d_btrans"):
            assert torch.equal(g[k], g2[k]), (cid, name, k, "two identical calls differ")
    assert not bad, bad


@pytest.mark.parametrize("cid,key,kw", _SPECS["options"], ids=_ids)
def test_lbs_options_against_float64(cid, key, kw, dmodel):
    """theta_mask, per-frame btrans / log-scales with and without propagate_scaling, allow_limb_scaling off, rotation-matrix
    poses, upstream gradients on Rs and v_shaped, del_v with shared betas, a custom template, nB_used below the model's nB on
    both sides of the k_shape_blend<8|16|0> and k_lbs_bwd_ndc<3|6|9> templates, pose blend shapes at a B that is no multiple of
    PB_FRAMES."""
    eng = _eng()
    t, dm = dmodel(key)
    case = r64.build_case(t, kw)
    ref_f, ref_g = r64.reference(t, case)
    routes = _routes(eng, dm, case)
    if key == "nb20":
        assert case["nB_used"] < t.nB
        if case["up"]["views"]:  # (more than nine coefficients do not fit the fused kernel's registers: the separate route)
            assert (len(routes) == 2) == (case["nB_used"] <= 9), (case["nB_used"], routes)
    bad = []
    for name, fused in routes:
        fwd, g = _run(dm, case, fused)
        bad += _errors(f"{cid}/{name}", fwd, g, ref_f, ref_g, case)
        if not case["fl"]["allow_limb_scaling"]:
            assert g["d_logscale"] is None and bool(ref_g["d_logscale"].eq(0).all())
        if "theta_mask" in case["inp"]:  # (d_theta is the gradient on theta * mask, masked axes included: see lbs_ref64.reference)
            assert bool((case["inp"]["theta_mask"] == 0).any()) and bool((case["inp"]["theta_mask"] == 1).any())
    assert not bad, bad


@pytest.mark.parametrize("cid,key,kw", _SPECS["pose"], ids=_ids)
def test_lbs_pose_edges_against_float64(cid, key, kw, dmodel):
    """One edge per frame (lbs_ref64.edge_theta): theta = 0, 1e-6 randn and 1e-3 randn (the ``theta + 1e-8`` of the reference's
    Rodrigues formula decides the axis), |theta| = pi - 1e-3, pi, pi + 0.5, 2 pi + 0.1 on random axes, a single-axis pose; with
    log-scales of 0.3 randn and of 1.0 randn."""
    eng = _eng()
    t, dm = dmodel(key)
    case = r64.build_case(t, kw)
    ref_f, ref_g = r64.reference(t, case)
    assert all(bool(torch.isfinite(v).all()) for v in ref_g.values())
    bad = []
    for name, fused in _routes(eng, dm, case):
        fwd, g = _run(dm, case, fused)
        bad += _errors(f"{cid}/{name}", fwd, g, ref_f, ref_g, case)
    assert not bad, bad


@pytest.mark.parametrize("views", [0, 1])
def test_lbs_backward_adds_to_or_fills_the_buffers_it_is_given(views, dmodel):
    """``d_beta_accum``: the old content plus the gradient; ``out_logscale`` / ``out_btrans``: overwritten with the gradient.
    The pre-filled shape gradient is half the reference's, so that neither part hides the other."""
    t, dm = dmodel("stick")
    case = r64.build_case(t, dict(B=6, seed=50 + views, views=views))
    _, ref_g = r64.reference(t, case)
    for name, fused in _routes(_eng(), dm, case):
        old = (0.5 * ref_g["d_beta"]).float()
        acc, out_ls, out_bt = old.to(DEV), torch.full((t.J, 3), 7.0, device=DEV), torch.full((t.J, 3), float("nan"), device=DEV)
        _, g = _run(dm, case, fused, d_beta_accum=acc, out_logscale=out_ls, out_btrans=out_bt)
        assert g["d_beta"] is acc and g["d_logscale"] is out_ls and g["d_btrans"] is out_bt
        for k, want in (("d_beta", old.double() + ref_g["d_beta"]), ("d_logscale", ref_g["d_logscale"]), ("d_btrans", ref_g["d_btrans"])):
            err = r64.row_err(g[k], want, 1)
            print(f"{name:10s} {k:11s} {err:.3e}  (bound {r64.TOL[k]:.1e})")
            assert err <= r64.TOL[k], (name, k, err)


def test_lbs_backward_decodes_packed_vertex_gradients(dmodel):
    """The fused backward on a ``d_ndc`` left as ``x * 2^32 + y`` fixed-point words with per-image factors (some 0: plain
    floats), negative y included, against float64 on the values the words encode."""
    eng = _eng()
    t, dm = dmodel("stick")
    case = r64.build_case(t, dict(B=5, seed=52, views=2))
    N = 10
    sc = torch.full((N,), 2.0 ** -30)
    sc[2::3] = 0.0
    words, dec = r64.encode_packed(case["up"]["d_ndc"].numpy(), sc.numpy())
    case["up"]["d_ndc"] = dec.float()
    assert torch.equal(case["up"]["d_ndc"].double(), dec) and bool((dec[..., 1] < 0).any())
    _, ref_g = r64.reference(t, case)
    cams = _cams(case["up"])
    kw = dict(trans=case["inp"]["trans"].to(DEV), logscale=case["inp"]["ls"].to(DEV), btrans=case["inp"]["bt"].to(DEV), **case["fl"])
    out = eng.lbs_forward(dm, case["inp"]["beta"].to(DEV), case["inp"]["theta"].to(DEV), project=dict(cams=cams), **kw)
    fov_img = torch.zeros(N, device=DEV)
    g = eng.lbs_backward(dm, out, None, None, ndc_upstream=dict(cams=cams, d_ndc=words.to(DEV), d_ndc_scale=sc.to(DEV),
                                                                   d_yx=case["up"]["d_yx"].to(DEV), d_fov_img=fov_img))
    g["d_fov"] = eng.fov_reduce(cams, fov_img)
    bad = _errors("packed/fused", {}, g, {}, ref_g, case)
    assert not bad, bad


@pytest.mark.parametrize("cid,kw", r64.projection_specs(), ids=_ids)
def test_projection_against_float64(cid, kw):
    """k_project / k_project_bwd / k_fov_reduce: one point, the block boundaries at 255 / 256 / 257 points, two blocks and one
    point, two-set launches, 1 / 3 / 32 views, shared and per-image fov, aspect ratios, either upstream gradient alone,
    accumulation into a given d_pts, packed d_ndc rows among plain ones, points 0.05 in front of a camera plane."""
    eng = _eng()
    c = r64.make_projection_case(**kw)
    ref_f, ref_g, ref_fov = r64.projection_reference(c)
    frames, N, sets = c["frames"], c["frames"] * c["views"], c["sets"]
    dev = lambda x: None if x is None else x.to(DEV).contiguous()  # noqa: E731
    cams = eng.CameraSet(dev(c["R"]), dev(c["T"]), dev(c["fov"]), dev(c["aspect"]), c["views"], c["S"])
    fov_img = torch.zeros(N, device=DEV)
    sc = dev(c.get("d_ndc_scale"))
    d_ndc0 = dev(sets[0].get("d_ndc_words", sets[0]["d_ndc"]))
    got = []
    if len(sets) == 2:
        a, b = dev(sets[0]["pts"]), dev(sets[1]["pts"])
        ndc, yx = eng.project_verts_and_joints(cams, a, b)
        da, db = eng.project_backward_verts_and_joints(cams, a, d_ndc0, b, dev(sets[1]["d_yx"]), fov_img, d_ndc_scale=sc)
        got = [(dict(ndc=ndc[..., :2], ndc_z=ndc[..., 2]), dict(d_pts=da)), (dict(yx=yx), dict(d_pts=db))]
    else:
        pts = dev(sets[0]["pts"])
        ndc, yx = eng.project(cams, pts)
        only_ndc, only_yx = eng.project(cams, pts, want_yx=False), eng.project(cams, pts, want_ndc=False)
        assert only_ndc[1] is None and only_yx[0] is None and torch.equal(only_ndc[0], ndc) and torch.equal(only_yx[1], yx)
        buf = dev(sets[0]["d_pts0"]) if c["accumulate"] else None
        d_pts, _ = eng.project_backward(cams, pts, d_ndc=d_ndc0 if "ndc" in c["want"] else None, d_yx=dev(sets[0]["d_yx"]) if "yx" in c["want"] else None,
                                        d_pts=buf, d_fov_img=fov_img, accumulate=c["accumulate"], d_ndc_scale=sc)
        assert buf is None or d_pts is buf
        got = [(dict(ndc=ndc[..., :2], ndc_z=ndc[..., 2], yx=yx), dict(d_pts=d_pts))]
    d_fov = eng.fov_reduce(cams, fov_img)
    torch.cuda.synchronize()
    sfx, bad = ("_near" if c["near"] else ""), []
    items = [("d_fov", d_fov, ref_fov, frames if ref_fov.numel() == N else 1)]
    for i, (f, g) in enumerate(got):
        items += [(k, v, {**ref_f[i], **ref_g[i]}[k], frames) for k, v in {**f, **g}.items()]
    for k, v, want, rows in items:
        err = r64.row_err(v, want, rows)
        print(f"{cid:24s} {k + sfx:12s} {err:.3e}  (bound {r64.TOL[k + sfx]:.1e})")
        if not err <= r64.TOL[k + sfx]:
            bad.append((cid, k + sfx, err, r64.TOL[k + sfx]))
    assert not bad, bad
