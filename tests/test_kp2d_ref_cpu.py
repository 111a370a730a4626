"""The float64 restatement of the multi-view 2-D keypoint term (tests/kp2d_ref.py) checked on the CPU before the GPU tests rely on it:
against ``fit_ref.joint_term`` (the reference's joint loss) on the same projections, against central differences, against the OpenCV
pinhole model through ``cameras.opencv_to_pinhole_camera``, its seen rule, and - for every seeded problem of tests/kp2d_cases.py the
GPU file measures row errors on - that the restatement evaluated in float32 stays within TOL / 16 of the float64 one (no reference row
has a near-cancelled maximum)."""
import numpy as np
import pytest
import torch

import fit_ref
import joints_cases
import kp2d_cases
import kp2d_ref
import pinhole_ref
from lbs_ref64 import MEASURED, row_err
from smilify_amd import cameras

F64 = torch.float64


@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("window", [3, 0])
def test_term_equals_the_joint_loss_on_the_same_projections(tables, views, window):
    """rho = s, no weights, no confidences: ``fit_ref.joint_term`` over all views, ragged (7 frames in windows of 3) and single windows.
    Bound 1e-12 relative (two float64 summation orders of ~100 terms)."""
    t = joints_cases.get_model("mouse", tables)
    N = 7
    p = kp2d_cases.problem(t, N, views, 11 + views)
    r = kp2d_cases.reference(t, p, 25.0, 0.0, window, weights=False)
    yx_all, z = kp2d_ref.project(r["joints"], p["cams"], p["S"], views)
    seen = kp2d_ref.seen_entries(p["target"], z[:, :, p["canon"]])
    assert torch.equal(seen, r["seen"]) and 0 < int(seen.sum()) < seen.numel()
    Jc = len(p["canon"])
    tgt = torch.where(torch.isfinite(p["target"]), p["target"], torch.zeros(())).reshape(N * views, Jc, 2)
    want, _, _ = fit_ref.joint_term(yx_all.reshape(N * views, t.J, 2), tgt, seen.reshape(N * views, Jc), 25.0, views, window, canon=p["canon"])
    rel = abs(r["term2d"].item() - want.item()) / abs(want.item())
    print(f"[kp2d-ref] views {views} window {window}: term {r['term2d'].item():.6e}, joint_term {want.item():.6e}, rel {rel:.1e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("sigma_px", [0.0, 2.0])
def test_gradient_agrees_with_central_differences(tables, sigma_px):
    """d term / d joints by autograd against (f(x + h d) - f(x - h d)) / 2h along random directions, float64.  Bound 1e-6 of the derivative:
    truncation h^2 f''' / 6 and rounding 1e-16 |f| / h at h = 1e-6 .. 1e-5 model units."""
    t = joints_cases.get_model("mouse", tables)
    p = kp2d_cases.problem(t, 6, 2, 5)
    joints = kp2d_cases.reference(t, p, 1.0, 0.0, 3)["joints"]
    f = lambda j: kp2d_ref.kp2d_term(j, p["cams"], p["S"], p["target"], p["vis"], p["conf"], p["wj"], p["canon"], 25.0, sigma_px, 3)  # noqa: E731
    x = joints.clone().requires_grad_()
    f(x).backward()
    g = torch.Generator().manual_seed(3)
    for k in range(4):
        d = torch.randn(joints.shape, generator=g, dtype=F64)
        want = float((x.grad * d).sum())
        errs = [abs(float(f(joints + h * d) - f(joints - h * d)) / (2 * h) - want) / abs(want) for h in (1e-5, 1e-6)]
        print(f"[kp2d-ref] sigma {sigma_px} direction {k}: d = {want:.6e}, finite-difference error {errs}")
        assert min(errs) < 1e-6, (k, want, errs)


def test_opencv_calibration_on_any_square_size():
    """A non-square calibration (1280 x 720, principal point off centre) through ``opencv_to_pinhole_camera`` at S = 500 - neither image
    side: yx equals ``pinhole_ref.pinhole_pixels`` to 1e-9 px."""
    g = np.random.default_rng(4)
    S = 500
    K = np.array([[1100.0, 0.0, 655.5], [0.0, 1085.0, 341.25], [0.0, 0.0, 1.0]])
    a = g.normal(size=3)
    a = a / np.linalg.norm(a) * 0.7
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R_cv = np.eye(3) + np.sin(0.7) / 0.7 * Kx + (1 - np.cos(0.7)) / 0.49 * Kx @ Kx
    t_cv = np.array([0.1, -0.2, 4.0])
    X = g.normal(size=(40, 3)) * 0.5
    # (float64 tables: the conversion's own float32 rounding of R and T is not what is measured here)
    flip = np.diag([-1.0, -1.0, 1.0])
    R32, T32, fov, aspect, pp = cameras.opencv_to_pinhole_camera(R_cv, t_cv, K, S)
    R, T = R_cv.T @ flip, flip @ t_cv
    assert np.abs(R - R32).max() < 1e-6 and np.abs(T - T32).max() < 1e-6
    cams = dict(R=torch.from_numpy(R)[None], T=torch.from_numpy(T)[None], fov=torch.tensor([fov], dtype=F64),
                aspect=torch.tensor([aspect], dtype=F64), principal=torch.from_numpy(pp)[None])
    yx, z = kp2d_ref.project(torch.from_numpy(X)[None], cams, S, 1)
    u, v = pinhole_ref.pinhole_pixels(X, R_cv, t_cv, K)
    err = max(np.abs(yx[0, 0, :, 1].numpy() - u).max(), np.abs(yx[0, 0, :, 0].numpy() - v).max())
    print(f"[kp2d-ref] opencv pinhole at S={S}: max |yx - (v,u)| = {err:.2e} px")
    assert err <= 1e-9 and bool((z > 0).all())


def test_seen_rule():
    """One joint, three views, four keypoints: a NaN coordinate, confidence 0 and NaN, and a joint behind the second camera - each
    contributes exactly 0 and no gradient; the rest are seen."""
    R, T = cameras.look_at_view_transform([3.0, 3.0, 3.0], [10.0, 10.0, 10.0], [0.0, 120.0, 240.0])
    cams = dict(R=R, T=T, fov=torch.tensor([40.0]))
    joints = torch.tensor([[[0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1], [0.0, 0.0, 0.0]]], dtype=F64)
    c1 = kp2d_cases.camera_centres(cams, 3)[1]
    joints[0, 3] = 1.2 * c1  # 0.6 behind camera 1, in front of the others
    yx, z = kp2d_ref.project(joints, cams, 128, 3)
    assert z[0, 1, 3] < -0.1 and bool((z[0, [0, 2], 3] > 1.0).all())
    target = (yx + 3.0).float()
    conf = torch.ones(1, 3, 4)
    target[0, 0, 0, 1] = float("nan")
    conf[0, 0, 1] = 0.0
    conf[0, 2, 1] = float("nan")
    want = torch.ones(1, 3, 4, dtype=torch.bool)
    want[0, 0, 0] = want[0, 0, 1] = want[0, 2, 1] = want[0, 1, 3] = False
    x = joints.clone().requires_grad_()
    term, yx_out, seen = kp2d_ref.kp2d_term(x, cams, 128, target, None, conf, None, None, 1.0, 0.0, 0, with_projection=True)
    term.backward()
    assert torch.equal(seen, want)
    assert bool(torch.isnan(yx_out[0, 1, 3]).all()) and int(torch.isnan(yx_out).sum()) == 2
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(term))
    # 8 seen entries, each 3 px off in y and x
    assert abs(term.item() - 8 * 18.0 / (2 * 4 * 3)) < 1e-3
    only = want.clone()
    only[0, 0] = False  # view 0 dropped through the visibility: joints 0 and 1 keep views (1, 2) and (1)
    x2 = joints.clone().requires_grad_()
    kp2d_ref.kp2d_term(x2, cams, 128, target, only, conf, None, None, 1.0, 0.0, 0).backward()
    assert bool((x2.grad[0, 0] != 0).any()) and bool((x.grad[0, 3] != 0).any())


# (with the sigma the GPU file runs them at: both for the N = 7 problems, 2 px for the block-loop ones)
ALL_PROBLEMS = [(k, 7, v, pi, ap, seed, sg) for k, v, pi, ap, seed in kp2d_cases.GPU_PROBLEMS for sg in (0.0, 2.0)] + \
    [(k, n, v, pi, True, seed, 2.0) for k, n, v, pi, seed in kp2d_cases.BLOCK_PROBLEMS]


@pytest.mark.parametrize("key,N,views,per_image,aspect_pp,seed,sigma_px", ALL_PROBLEMS)
def test_float32_restatement_stays_within_a_sixteenth_of_the_bounds(tables, key, N, views, per_image, aspect_pp, seed, sigma_px):
    """The problems of tests/test_gpu_fit_keypoints2d.py: row_err(float32 restatement, float64 restatement) <= TOL / 16 (=
    ``lbs_ref64.MEASURED``) for every quantity the GPU test bounds by TOL.  A seed that fails this is replaced, never the bound."""
    t = joints_cases.get_model(key, tables)
    p = kp2d_cases.problem(t, N, views, seed, per_image, aspect_pp)
    _float32_check(t, p, N, sigma_px, f"{key} views {views} per_image {per_image} sigma {sigma_px}", skip=("d_logscale",) if key == "j3" else ())


def _float32_check(t, p, N, sigma_px, name, weights=True, w_k3d=0.0, sigma=0.0, skip=()):
    r64, r32 = (kp2d_cases.reference(t, p, 25.0, sigma_px, 3, weights, w_k3d=w_k3d, sigma=sigma, dtype=d) for d in (F64, torch.float32))
    rows = dict(d_theta=("pose", N), d_trans=("trans", N), d_beta=("betas", 1), d_logscale=("log_beta_scales", 1), d_btrans=("betas_trans", 1))
    for k in skip:  # (j3: its joints do not depend on the log scales beyond rounding - the GPU file freezes that table there)
        rows.pop(k)
    errs = {k: row_err(r32["grads"][n], r64["grads"][n], m) for k, (n, m) in rows.items()}
    fin = torch.isfinite(r64["yx"])
    assert torch.equal(fin, torch.isfinite(r32["yx"]))
    errs["yx"] = row_err(torch.where(fin, r32["yx"], torch.zeros(())), torch.where(fin, r64["yx"], torch.zeros((), dtype=F64)), N)
    errs["joints"] = row_err(r32["joints"], r64["joints"], N)
    print(f"[kp2d-ref] float32 restatement {name}: " + " ".join(f"{k} {v:.1e}/{MEASURED[k]:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= MEASURED[k], (k, v, MEASURED[k])


@pytest.mark.parametrize("kw", kp2d_cases.BOTH_PROBLEMS, ids=lambda kw: f"{kw['key']}-{kw['seed']}")
@pytest.mark.parametrize("weights", [True, False])
def test_float32_restatement_of_both_terms(tables, kw, weights):
    """The problems of ``test_both_terms`` with the weights it uses: both terms evaluated in float32."""
    kw = dict(kw)
    t = joints_cases.get_model(kw.pop("key"), tables)
    p = kp2d_cases.problem(t, kw.pop("N"), kw.pop("views"), kw.pop("seed"), **kw)
    _float32_check(t, p, p["N"], 2.0, f"both terms {p['N']} w{int(weights)}", weights, w_k3d=2e6 / p["length"] ** 2, sigma=0.05)


@pytest.mark.parametrize("kw", kp2d_cases.SHIPPED_PROBLEMS, ids=lambda kw: f"{kw['key']}-{kw['seed']}")
def test_float32_restatement_of_the_shipped_fitter_problems(tables, kw):
    """The problems of ``test_against_the_shipped_fitter`` (rho = s, no weights)."""
    kw = dict(kw)
    t = joints_cases.get_model(kw.pop("key"), tables)
    p = kp2d_cases.problem(t, kw.pop("N"), kw.pop("views"), kw.pop("seed"), **kw)
    _float32_check(t, p, p["N"], 0.0, f"shipped views {p['views']}", weights=False)


@pytest.mark.parametrize("sigma_px", [0.0, 2.0])
def test_float32_restatement_of_the_single_joint_problem(tables, sigma_px):
    t = joints_cases.get_model("j3_static", tables)
    p = kp2d_cases.single_joint_problem(t, kp2d_cases.SINGLE_JOINT_SEED)
    _float32_check(t, p, p["N"], sigma_px, f"single joint sigma {sigma_px}")
