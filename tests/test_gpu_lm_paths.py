"""The rules of csrc/lm.h on the GPU, step by step, in both kernels that run them: the point refinement (engine.refine_points on
csrc/refine_points.hip, lm_solve<3> in registers, the loop inside the kernel) and the camera refinement (engine.refine_cameras on
csrc/refine.hip, lm_solve<6 | 10> in LDS, a host loop that polls every 8 pairs).  The cases are those of tests/lm_cases.py;
tests/test_lm_paths_cpu.py proves on the restatement that together they take every branch.

Prefix runs.  A run with max_steps = k returns the state after k evaluations, so for every k of a case's safe prefix (lm_cases.prefix_steps)
status, n_accepted and n_trials are the restatement's exactly, and cost0, cost and the point or parameters are within
max(4 x the restatement's own error, 2^-45) of the exact-step iteration (lm_ref.lm_exact: every evaluation and solve in 40 digits) at
the same prefix: the rule and the floor of test_gpu_refine_kernels.py and test_gpu_refine_points_kernels.py.  The error is relative
for a cost, in units of the largest entry for a point and refine_ref.rotation_distance (R, t, K) for a camera.  The cost of a prefix
has one more admitted term, derived at check_prefix, and is in exchange held to the 40-digit cost of its own point.  Past the safe prefix
the run goes to its end once: status CONVERGED and the restatement's final cost to 1e-9, the bound of test_gpu_refine.py.

The exact cases (a system lm_solve refuses for N = 3, 6, 10; a cost of exactly 0) have counts that follow from the rules alone:
9, 9, 9 and 17 trials, none accepted, CONVERGED, every output the input to the bit."""
import numpy as np
import pytest

import lm_cases as C
import lm_ref as L
import refine_points_ref as RP
import refine_ref as RC
from test_gpu_refine_points_kernels import same_fit

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -45
POINTS = {c["name"]: c for c in C.POINT_CASES}
CAMERAS = {c["name"]: c for c in C.CAMERA_CASES}
BESIDE_MANY = ("mild", "many", "flat")  # the 300-point camera between two of 24: two accumulation workgroups per camera


# ---- the two entry points ----
def run_points(cases, max_steps=C.POINT_STEPS):
    """engine.refine_points (through refine_points_arrays) on the problems `cases` as one launch: (xyz (N,1,3), stats)."""
    from smilify_amd import refine_points as rp

    obs = np.stack([c["obs"] for c in cases])[:, None]
    mask = np.array([c["mask"] for c in cases], np.uint32)[:, None]
    xyz0 = np.stack([c["xyz0"] for c in cases])[:, None]
    return rp.refine_points_arrays(C.POINT_P, obs, mask, xyz0, C.F_SCALE, max_steps)


def run_cameras(cases, n_params, max_steps=C.CAMERA_STEPS):
    """engine.refine_cameras on the cameras `cases` as one launch: dict of params, status, n_accepted, n_trials, cost0, cost, g."""
    from smilify_amd import engine
    from smilify_amd import triangulate as tri

    dev = engine.require_gpu(tri.DEFAULT_DEVICE)
    up = lambda x: engine.upload_f64(np.ascontiguousarray(x, np.float64), dev)  # noqa: E731
    offsets = np.concatenate([[0], np.cumsum([len(c["p3"]) for c in cases])]).astype(np.int64)
    out = engine.refine_cameras(up(np.concatenate([c["p3"] for c in cases])), up(np.concatenate([c["p2"] for c in cases])), offsets,
                                up(np.stack([c["start"] for c in cases])), n_params=n_params, f_scale=C.F_SCALE, max_steps=max_steps)
    return dict(zip(("params", "status", "n_accepted", "n_trials", "cost0", "cost", "g"), (t.cpu().numpy() for t in out)))


def camera_alone(out, i):
    return {k: v[i:i + 1] for k, v in out.items()}


def same_cameras(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- the bounds ----
def cost_error(c, exact):
    return abs(c - exact) / abs(exact) if exact != 0.0 else (0.0 if c == 0.0 else np.inf)


def check_prefix(label, k, got, ref, exact, distance, costs_at, worst):
    """got, the restatement and the exact-step iteration after k evaluations.  distance(x, x_exact) returns a tuple; costs_at(x) the
    40-digit cost at x and numpy's.

    The cost of a prefix has a third term in its bound, because away from the minimum it is not an independent quantity.  An
    implementation whose current point is x_exact + d returns, to first order, cost(x_exact) + g . d.  For the restatement that IS its cost
    error (measured on `far`: |g . d| / cost and the cost error agree to two digits at every k), and g . d is a signed sum whose terms
    cancel by a factor 10 to 1000, so 4 x the restatement's cost error at one k is 4 x one sample of that cancellation: at k = 10 of `far`
    it is 1.4e-12, at k = 47 3.9e-14, with the same 1.5e-13 error of the parameters.  What the point bound allows d to be, 4 |d_ref|
    entry by entry, allows the cost sum_i |g_i| 4 |d_ref,i| / cost: a kernel inside the point bound cannot be held to less.  At a minimum
    g = 0 and the term vanishes.  So that the cost is still held to the float64 of ITS OWN point, it is also compared with the 40-digit
    cost evaluated at the returned point, by the rule of the accumulation tests: max(4 x numpy's error there, 2^-45)."""
    p_ref, p_exact = L.prefix(ref, k), L.prefix(exact, k)
    assert (got["status"], got["n_accepted"], got["n_trials"]) == (p_ref["status"], p_ref["n_accepted"], p_ref["n_trials"]), (label, k, got, p_ref)
    first_order = 4.0 * float(np.abs(p_exact["g"]) @ np.abs(p_ref["x"] - p_exact["x"])) / p_exact["cost"] if p_exact["cost"] else 0.0
    pairs = [("cost0", cost_error(got["cost0"], p_exact["cost0"]), cost_error(p_ref["cost0"], p_exact["cost0"]), 0.0),
             ("cost", cost_error(got["cost"], p_exact["cost"]), cost_error(p_ref["cost"], p_exact["cost"]), first_order)]
    pairs += [(name, g, r, 0.0) for name, g, r in zip(("x", "t", "K") if len(distance(p_ref["x"], p_exact["x"])) == 3 else ("x",),
                                                      distance(got["x"], p_exact["x"]), distance(p_ref["x"], p_exact["x"]))]
    at_40, at_numpy = costs_at(got["x"])
    pairs.append(("cost at its own point", cost_error(got["cost"], at_40), cost_error(at_numpy, at_40), 0.0))
    print(f"{label} k = {k}: " + ", ".join(f"{name} gpu {g:.2e} restatement {r:.2e}" for name, g, r, _ in pairs) + f", 4 sum |g| |d| / cost {first_order:.2e}")
    for name, g, r, extra in pairs:
        kind = "own" if name.endswith("own point") else ("cost" if name.startswith("cost") else "x")
        if g > worst[kind][0]:
            worst[kind] = (g, r, f"{label} k = {k} {name}")
        assert g <= max(4.0 * r, FLOOR, extra), (label, k, name, g, r, extra)


def check_tail(label, got, ref, safe):
    """Past the safe prefix: the run to its end."""
    print(f"{label}: trials gpu {got['n_trials']} restatement {ref['n_trials']}, accepted gpu {got['n_accepted']} restatement {ref['n_accepted']}, "
          f"safe prefix {safe}, final cost gpu / restatement - 1 = {got['cost'] / ref['cost'] - 1 if ref['cost'] else 0.0:.2e}")
    if safe == ref["n_trials"]:
        return  # the run ends inside its safe prefix: the prefix run at k = safe has asserted everything
    assert got["status"] == L.CONVERGED == ref["status"], label
    assert abs(got["cost"] - ref["cost"]) <= 1e-9 * ref["cost"], label
    assert got["n_trials"] >= safe and got["n_accepted"] >= L.prefix(ref, safe)["n_accepted"]


# ---- prefix runs ----
@pytest.mark.parametrize("name", [c["name"] for c in C.POINT_CASES])
def test_point_prefixes(name):
    case = POINTS[name]
    ref, exact = C.point_run(case)
    label, worst = "point " + name, dict(cost=(0.0, 0.0, ""), own=(0.0, 0.0, ""), x=(0.0, 0.0, ""))
    if exact is None:  # the start has no finite cost: one evaluation whatever the limit
        for k in (1, 2, C.POINT_STEPS):
            xyz, st = run_points([case], k)
            assert st["status"][0, 0] == L.NONFINITE and st["n_trials"][0, 0] == 1 and st["n_accepted"][0, 0] == 0
            assert np.array_equal(xyz[0, 0].view(np.int64), case["xyz0"].view(np.int64)) and not np.isfinite(st["cost_initial"][0, 0])
        return
    safe = L.safe_prefix(ref)
    assert safe >= case["min_safe"]

    def costs_at(x):
        return RP.evaluate_mp(C.POINT_P, case["obs"], case["mask"], x, C.F_SCALE)[0], RP.evaluate(C.POINT_P, case["obs"], case["mask"], x, C.F_SCALE)[0]

    for k in C.prefix_steps(safe):
        xyz, st = run_points([case], k)
        got = dict(x=xyz[0, 0], status=int(st["status"][0, 0]), n_accepted=int(st["n_accepted"][0, 0]), n_trials=int(st["n_trials"][0, 0]),
                   cost0=float(st["cost_initial"][0, 0]), cost=float(st["cost_final"][0, 0]))
        check_prefix(label, k, got, ref, exact, lambda a, b: (L.rel_err(a, b),), costs_at, worst)
    xyz, st = run_points([case])
    check_tail(label, dict(status=int(st["status"][0, 0]), n_accepted=int(st["n_accepted"][0, 0]), n_trials=int(st["n_trials"][0, 0]),
                           cost=float(st["cost_final"][0, 0])), ref, safe)
    print(f"{label}: largest errors over the safe prefix: cost gpu {worst['cost'][0]:.2e} restatement {worst['cost'][1]:.2e} ({worst['cost'][2]}); "
          f"cost at its own point gpu {worst['own'][0]:.2e} numpy {worst['own'][1]:.2e}; point gpu {worst['x'][0]:.2e} restatement {worst['x'][1]:.2e} ({worst['x'][2]})")


@pytest.mark.parametrize("name,n_params", [(c["name"], n) for c, n in C.CAMERA_RUNS])
def test_camera_prefixes(name, n_params):
    case = CAMERAS[name]
    ref, exact = C.camera_run(case, n_params)
    label, worst = f"camera {name} p{n_params}", dict(cost=(0.0, 0.0, ""), own=(0.0, 0.0, ""), x=(0.0, 0.0, ""))
    cases = [CAMERAS[n] for n in BESIDE_MANY] if name == "many" else [case]
    i = cases.index(case)
    if exact is None:  # skipped, or a start without a finite cost: nothing moves whatever the limit
        for k in (1, 2, 9, C.CAMERA_STEPS):
            out = run_cameras(cases, n_params, k)
            assert out["status"][i] == ref["status"] and out["n_trials"][i] == ref["n_trials"] and out["n_accepted"][i] == 0
            assert np.array_equal(out["params"][i].view(np.int64), case["start"].view(np.int64)) and not out["g"][i].any()
            assert not np.isfinite(out["cost0"][i]) and not np.isfinite(out["cost"][i])
        return
    safe = L.safe_prefix(ref)
    assert safe >= case["min_safe"][n_params]

    def costs_at(x):
        return RC.evaluate_mp(x, case["p3"], case["p2"], C.F_SCALE)[0], RC.evaluate(x, case["p3"], case["p2"], n_params, C.F_SCALE)[0]

    def one(k):
        out = run_cameras(cases, n_params, k)
        return dict(x=out["params"][i], status=int(out["status"][i]), n_accepted=int(out["n_accepted"][i]), n_trials=int(out["n_trials"][i]),
                    cost0=float(out["cost0"][i]), cost=float(out["cost"][i]))

    for k in C.prefix_steps(safe):
        check_prefix(label, k, one(k), ref, exact, RC.rotation_distance, costs_at, worst)
    check_tail(label, one(C.CAMERA_STEPS), ref, safe)
    print(f"{label}: largest errors over the safe prefix: cost gpu {worst['cost'][0]:.2e} restatement {worst['cost'][1]:.2e} ({worst['cost'][2]}); "
          f"cost at its own point gpu {worst['own'][0]:.2e} numpy {worst['own'][1]:.2e}; R, t or K gpu {worst['x'][0]:.2e} restatement {worst['x'][1]:.2e} ({worst['x'][2]})")


# ---- exact cases ----
@pytest.mark.parametrize("name,trials", [("singular", 9), ("zero_cost", 17)])
def test_exact_point_cases(name, trials):
    """Every evaluation after the first is of the start again, bit for bit, and is rejected: nothing may move and nothing may be accepted
    (a `<=` in lm_judge would accept every one of them; a fallback without its x10 would need 17 trials, not 9)."""
    case = POINTS[name]
    xyz, st = run_points([case])
    assert (int(st["status"][0, 0]), int(st["n_trials"][0, 0]), int(st["n_accepted"][0, 0])) == (L.CONVERGED, trials, 0)
    assert st["cost_final"][0, 0].tobytes() == st["cost_initial"][0, 0].tobytes() and np.isfinite(st["cost_initial"][0, 0])
    assert np.array_equal(xyz[0, 0].view(np.int64), case["xyz0"].view(np.int64))
    if name == "zero_cost":
        assert st["cost_initial"][0, 0] == 0.0 and not st["view_err"][0, 0, 6:9].any()
    short = run_points([case], trials - 1)[1]
    assert (int(short["status"][0, 0]), int(short["n_trials"][0, 0])) == (L.STEP_LIMIT, trials - 1)  # not one evaluation sooner


@pytest.mark.parametrize("name,n_params", [("flat", 10), ("fy_zero", 6), ("fy_zero", 10)])
def test_exact_camera_cases(name, n_params):
    """H has a row of exact zeros inside the fitted block (row 6 for `flat`, row 4 for `fy_zero`), so lm_solve<N> meets a pivot of exactly
    0 every time: 9 trials, each x100 on lambda, none accepted, the parameters the start's to the bit, and g what one accumulation gives."""
    from smilify_amd import refine_cameras as rc

    case = CAMERAS[name]
    out = run_cameras([case], n_params)
    assert (int(out["status"][0]), int(out["n_trials"][0]), int(out["n_accepted"][0])) == (L.CONVERGED, 9, 0)
    assert out["cost"][0].tobytes() == out["cost0"][0].tobytes() and np.isfinite(out["cost0"][0])
    assert np.array_equal(out["params"][0].view(np.int64), case["start"].view(np.int64))
    cost, g, H = rc.evaluate_cost(case["start"][None], [(case["p3"], case["p2"])], optimize_intrinsics=n_params == 10, f_scale=C.F_SCALE)
    assert np.array_equal(out["g"][0], g[0]) and g[0][:n_params].any()
    row = 6 if name == "flat" else 4
    assert not H[0][row].any() and not H[0][:, row].any()  # the kernel's own H has the exact zeros the case is built on
    short = run_cameras([case], n_params, 8)
    assert (int(short["status"][0]), int(short["n_trials"][0])) == (L.STEP_LIMIT, 8)


# ---- mixed launches ----
MIXED_POINTS = ("no_cost", "singular", "outlier", "zero_cost", "rejecting", "all_views", "no_cost", "singular", "outlier", "zero_cost", "rejecting")


def test_points_of_every_path_in_one_launch():
    """11 problems, three workgroups of RPT_WAVES = 4 waves, the last partly filled; the first holds problems that leave the loop after
    1, 9, 10 and 17 evaluations.  Each gives the bits of its run alone."""
    batch = run_points([POINTS[n] for n in MIXED_POINTS])
    trials = batch[1]["n_trials"][:4, 0].tolist()
    assert trials[0] == 1 and trials[1] == 9 and trials[3] == 17 and 9 <= trials[2] <= 12 and len(MIXED_POINTS) % 4 == 3
    alone = {n: run_points([POINTS[n]]) for n in set(MIXED_POINTS)}
    for i, n in enumerate(MIXED_POINTS):
        assert same_fit(alone[n], batch, slice(i, i + 1)), (i, n)


@pytest.fixture(scope="module")
def mixed_cameras():
    """Every 24-point camera, the skipped one (19 points) and the start without a finite cost in one launch, for 10 and for 6
    parameters, at the step limits around the host's polls: once."""
    return {(n, k): run_cameras(C.SMALL_CAMERAS, n, k) for n in (10, 6) for k in (7, 8, 9, 15, 16, 17, 100)}


@pytest.mark.parametrize("n_params", [10, 6])
def test_cameras_of_every_path_in_one_launch(mixed_cameras, n_params):
    batch = mixed_cameras[(n_params, 100)]
    names = [c["name"] for c in C.SMALL_CAMERAS]
    assert batch["status"][names.index("few")] == RC.SKIPPED and batch["status"][names.index("nan_start")] == RC.NONFINITE
    assert batch["status"][names.index("stuck")] == (RC.STEP_LIMIT if n_params == 10 else RC.CONVERGED)
    assert len(set(batch["n_trials"].tolist())) >= 5  # cameras that are done at different pairs share every launch after that
    for i, c in enumerate(C.SMALL_CAMERAS):
        assert same_cameras(run_cameras([c], n_params), camera_alone(batch, i)), c["name"]


@pytest.mark.parametrize("n_params", [10, 6])
def test_a_camera_that_is_done_stays_as_it_is(mixed_cameras, n_params):
    """Done after t trials: identical bits for every max_steps >= t, on either side of a poll of the host."""
    full = mixed_cameras[(n_params, 100)]
    frozen = 0
    for k in (7, 8, 9, 15, 16, 17):
        out = mixed_cameras[(n_params, k)]
        for i, c in enumerate(C.SMALL_CAMERAS):
            if full["status"][i] != RC.STEP_LIMIT and full["n_trials"][i] <= k:
                assert same_cameras(camera_alone(out, i), camera_alone(full, i)), (c["name"], k)
                frozen += 1
            else:
                assert out["status"][i] == RC.STEP_LIMIT and out["n_trials"][i] == k, (c["name"], k)
    assert frozen >= 12


def test_a_launch_that_is_done_before_the_first_poll():
    """Every camera is done within 8 pairs: the host's first poll ends the loop, and 100 allowed steps return the bits of 8."""
    cases = [CAMERAS[n] for n in ("near", "nan_start", "few")]
    at8, at100 = run_cameras(cases, 6, 8), run_cameras(cases, 6, 100)
    assert (at8["status"] != RC.STEP_LIMIT).all() and at8["n_trials"].max() <= 8
    assert same_cameras(at8, at100)
