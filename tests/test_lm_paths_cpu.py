"""The proof, without a GPU, that tests/test_gpu_lm_paths.py tests something: on the numpy restatement alone (tests/lm_ref.py) the cases of
tests/lm_cases.py together take every branch of csrc/lm.h, each case takes the path it is named for, each has the safe prefix it
declares, and inside that prefix the restatement takes the decisions of the exact-step iteration (every evaluation and solve in 40
digits).  Outside their safe prefixes the cases have at most 3 decisions each: the convergence tail, whose last decisions are close by
construction (the stop rule is "lowered by less than 1e-12")."""
import re

import numpy as np
import pytest

import lm_cases as C
import lm_ref as L
import refine_points_ref as RP
import refine_ref as RC

TAIL_CAP = 3


@pytest.fixture(scope="module")
def runs():
    return C.all_runs()


def safe_part(ref):
    return ref["trace"][:L.safe_prefix(ref)]


def judged(entries):
    """The decisions that compared two costs of two different points."""
    return [e for e in entries if e["decision"] in (L.ACCEPT, L.REJECT) and not e["exempt"]]


def refused_throughout(ref, x0):
    """9 evaluations of the start: each trial multiplies lambda by 100, the fallback's x10 and the rejection's x10."""
    t = ref["trace"]
    return (L.decisions(ref) == "srrrrrrrR" and ref["status"] == L.CONVERGED and ref["n_accepted"] == 0 and t[-1]["lam"] == pytest.approx(1e13)
            and all(e["exempt"] for e in t[1:]) and np.array_equal(np.asarray(ref.get("xyz", ref.get("params"))).view(np.int64), x0.view(np.int64))
            and ref["cost"] == ref["cost0"])


def test_margin_at_cost_zero_and_the_trace():
    """A start with cost exactly 0 used to divide by it.  The trace has one entry per evaluation."""
    ref, exact = C.point_run(C.POINT_CASES[2])
    assert C.POINT_CASES[2]["name"] == "zero_cost" and ref["cost0"] == 0.0 and ref["cost"] == 0.0 and ref["margin"] == np.inf
    assert len(ref["trace"]) == ref["n_trials"] == 17 and all(e["margin"] == 0.0 and e["exempt"] for e in ref["trace"][1:])
    for out in (ref, exact):
        for k in (1, 5, 17, 30):
            p = L.prefix(out, k)
            assert p["n_trials"] == min(k, 17) and p["status"] == (L.CONVERGED if k >= 17 else L.STEP_LIMIT)
    assert set(ref["trace"][0]) >= {"cost", "decision", "refused", "lam", "x", "margin", "exempt"}


def test_prefix_is_the_run_with_a_smaller_step_limit():
    c = C.POINT_CASES[0]
    ref = C.point_run(c)[0]
    for k in (1, 2, 5, 14, 16, 40):
        short, p = RP.lm(C.POINT_P, c["obs"], c["mask"], c["xyz0"], C.F_SCALE, k), L.prefix(ref, k)
        assert np.array_equal(short["xyz"], p["x"]) and all(short[f] == p[f] for f in ("status", "n_accepted", "n_trials", "cost0", "cost")), k


def test_every_branch_of_lm_h_is_reached(runs):
    safe = [(label, ref, safe_part(ref)) for label, ref, exact, path, m in runs]
    seq = {label: L.decisions(dict(trace=part)) for label, ref, part in safe}
    every = [e for _, _, part in safe for e in part]
    print("\n".join(f"{label}: {L.decisions(ref)} safe prefix {len(part)}" for label, ref, part in safe))
    assert any(e["decision"] == L.START for e in every)                                    # lm_judge: fresh, finite
    assert any(e["decision"] == L.ACCEPT for e in judged(every))                           # lm_judge: cost_new < cost_cur
    assert any(e["decision"] == L.REJECT for e in judged(every))                           # lm_judge: else
    for kernel in ("point", "camera"):
        mine = [s for label, s in seq.items() if label.startswith(kernel)]
        assert any("RA" in s for s in mine) and any("AR" in s for s in mine), kernel         # an accept directly after a reject, and the reverse
    assert any(re.search("A{9,}.*R", L.decisions(ref)) for _, ref, _ in safe)               # nine accepts in a row, and a reject after them
    assert any(e["lam"] <= 1e-12 * (1.0 + 1e-9) for _, ref, _ in safe for e in ref["trace"])  # the floor itself
    for n, who in ((3, "point singular"), (6, "camera fy_zero p6"), (10, "camera flat p10")):  # lm_solve<N> refuses
        assert any(label == who and any(e["refused"] for e in part) for label, _, part in safe), n
    assert any(ref["status"] == L.CONVERGED and ref["trace"][-1]["decision"] == L.ACCEPT and ref["trace"][-1]["lam"] < 1.0 for _, ref, _ in safe)  # the 1e-12 rule
    rejects_alone = [ref for _, ref, _ in safe if ref["status"] == L.CONVERGED and ref["trace"] and ref["trace"][-1]["lam"] > 1e12
                     and not any(e["refused"] for e in ref["trace"])]
    assert len(rejects_alone) == 1 and rejects_alone[0]["n_trials"] == 17                  # the ceiling through rejects alone
    fallback = [ref for _, ref, _ in safe if ref["status"] == L.CONVERGED and ref["trace"] and ref["trace"][-1]["lam"] > 1e12
                and any(e["refused"] for e in ref["trace"])]
    assert len(fallback) == 3 and all(ref["n_trials"] == 9 for ref in fallback)            # the ceiling through the fallback: x100 per trial
    assert any(ref["status"] == L.STEP_LIMIT and ref["n_trials"] == C.CAMERA_STEPS for _, ref, _ in safe)  # the whole step limit
    assert any(ref["status"] == L.NONFINITE and ref["n_trials"] == 1 and ref["trace"][0]["decision"] == L.NONFINITE_COST for _, ref, _ in safe)
    # what no case reaches (the lm.h paragraph): a non-finite cost after a finite start
    assert not any(e["decision"] == L.NONFINITE_COST for _, ref, _ in safe for e in ref["trace"][1:])


def test_each_case_takes_its_path(runs):
    by_label = {label: (ref, path) for label, ref, exact, path, m in runs}
    points = {c["name"]: c for c in C.POINT_CASES}
    cameras = {c["name"]: c for c in C.CAMERA_CASES}
    for label, (ref, path) in by_label.items():
        kind, name = label.split()[:2]
        case = points[name] if kind == "point" else cameras[name]
        x0 = case["xyz0"] if kind == "point" else case["start"]
        seq, part = L.decisions(ref), safe_part(ref)
        if path == "reject":
            assert re.fullmatch("SRRARA{9}RA", seq) and len(part) >= 13 and ref["status"] == L.CONVERGED
        elif path == "interleaved":
            rejects = [e for e in judged(part) if e["decision"] == L.REJECT]
            assert ref["status"] == L.CONVERGED and len(rejects) >= 20 and ref["n_trials"] > 56  # seven polls of the host
        elif path == "step_limit":
            assert ref["status"] == L.STEP_LIMIT and len(part) == ref["n_trials"] == C.CAMERA_STEPS and seq.count("R") >= 40
        elif path == "iterates":
            assert ref["status"] == L.CONVERGED and ref["trace"][-1]["decision"] == L.ACCEPT and not any(e["refused"] for e in ref["trace"])
            assert ref["n_accepted"] >= 4
        elif path in ("refused3", "refused6", "refused10"):
            assert refused_throughout(ref, x0), label
        elif path == "zero_cost":
            assert seq == "S" + "R" * 16 and ref["cost0"] == 0.0 and ref["status"] == L.CONVERGED and np.array_equal(ref["xyz"], x0)
        elif path == "outlier":
            v = RP.views_of(case["mask"], 32)
            f = RP.jacobian(C.POINT_P[v], ref["xyz"])[0] - case["obs"][v]
            w = 1.0 / np.sqrt(1.0 + (f / C.F_SCALE) ** 2)
            assert ref["status"] == L.CONVERGED and w.min() < 0.05 and w.max() > 0.9  # weights far from 1, and near it
        elif path == "lanes64":
            assert int(case["mask"]) == 0xFFFFFFFF and ref["status"] == L.CONVERGED
        elif path == "two_partials":
            assert len(case["p3"]) > 256 and ref["status"] == L.CONVERGED
        elif path == "nonfinite_start":
            assert ref["status"] == L.NONFINITE and ref["n_trials"] == 1 and not np.isfinite(ref["cost0"])
        elif path == "skipped":
            assert ref["status"] == RC.SKIPPED and ref["n_trials"] == 0 and len(case["p3"]) == RC.MIN_POINTS - 1
        else:
            raise AssertionError(f"{label}: no check for the path {path}")
    assert all(len(c["p3"]) == 24 for c in C.SMALL_CAMERAS if c["name"] != "few") and RC.MIN_POINTS == 20


def test_safe_prefixes_and_the_tail_cap(runs):
    for label, ref, exact, path, min_safe in runs:
        safe = L.safe_prefix(ref)
        tail = [e for e in ref["trace"][safe:] if e["decision"] in (L.ACCEPT, L.REJECT)]
        print(f"{label}: {ref['n_trials']} trials, safe prefix {safe} (declared {min_safe}), {len(tail)} decisions outside it, closest safe margin "
              f"{min([e['margin'] for e in judged(ref['trace'][:safe])], default=np.inf):.1e}")
        assert safe >= min_safe, label
        assert len(tail) <= TAIL_CAP, label
    assert C.prefix_steps(34) == list(range(1, 21)) + [23, 24, 25, 31, 32, 33, 34] and C.prefix_steps(9) == list(range(1, 10))


def test_restatement_takes_the_decisions_of_the_exact_step_iteration(runs):
    """Inside the safe prefix: decision by decision, refusal by refusal, with the restatement's point and cost near the exact ones
    (printed: they are the yardsticks of the GPU test)."""
    worst, room = dict(point=0.0, cost=0.0), np.inf
    for label, ref, exact, path, m in runs:
        if exact is None:
            continue
        safe = L.safe_prefix(ref)
        assert L.safe_prefix(exact) >= safe - 1, label  # (its own margins may differ in the last digit of a 1e-9)
        for k in range(safe):
            a, b = ref["trace"][k], exact["trace"][k]
            assert (a["decision"], a["refused"], a["exempt"], a["n_accepted"], a["done"]) == (b["decision"], b["refused"], b["exempt"], b["n_accepted"], b["done"]), (label, k)
            assert a["lam"] == b["lam"]
            err = abs(a["cost_cur"] - b["cost_cur"]) / abs(b["cost_cur"]) if b["cost_cur"] != 0.0 else 0.0
            if a["decision"] in (L.ACCEPT, L.REJECT) and not a["exempt"]:
                # a kernel at 4 x the restatement's error on both costs of this decision stays inside its margin
                before = ref["trace"][k - 1]["cost_cur"], exact["trace"][k - 1]["cost_cur"]
                both = err + abs(before[0] - before[1]) / abs(before[1])
                assert 4.0 * both < a["margin"], (label, k, both, a["margin"])
                room = min(room, a["margin"] / max(both, 2.0 ** -52))
            worst["cost"] = max(worst["cost"], err)
            worst["point"] = max(worst["point"], L.rel_err(a["x"], b["x"]) if label.startswith("point") else max(RC.rotation_distance(a["x"], b["x"])))
    print(f"restatement against the exact-step iteration over all safe prefixes: cost {worst['cost']:.2e}, point or (R, t, K) {worst['point']:.2e}")
    print(f"the closest safe decision is {room:.1e} restatement errors wide")
