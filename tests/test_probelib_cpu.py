"""tools/probelib.py without a device: the step runner against a fake probe, the window sizing and alternation against a fake
``window``, and the byte-for-byte comparison at the cases where the probes' earlier copies disagreed."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
sys.path.insert(0, TOOLS)
import probelib  # noqa: E402

FAKE_PROBE = '''
import json, os, signal, sys, time
step, forwarded, log = sys.argv[2], sys.argv[3:], os.path.join(os.path.dirname(os.path.abspath(__file__)), "log")
with open(log, "a") as f:
    f.write(f"{step} {os.getpid()}\\n")
def row(k):
    print("ROW " + json.dumps(dict(step=step, k=k, forwarded=forwarded)), flush=True)
if step in ("ok", "ok2"):
    row(0), row(1)
    print("DEVICE " + json.dumps(["device of " + step, "1.0"]), flush=True)
elif step == "bad":
    row(0)
    sys.exit(3)
elif step == "killed":
    os.kill(os.getpid(), signal.SIGKILL)
elif step == "slow":
    row(0)
    time.sleep(60)
'''
FORWARD = ["--window-ms", "20.0", "--batches", "64", "1"]


@pytest.fixture
def fake(tmp_path):
    script = tmp_path / "fake_probe.py"
    script.write_text(FAKE_PROBE)

    def log():
        return [line.split() for line in (tmp_path / "log").read_text().splitlines()]
    return str(script), log


def test_runner_collects_every_step_that_finishes(fake):
    script, log = fake
    rows, failed, device, finished = probelib.run_steps(script, ["ok", "ok2"], FORWARD, 30)
    assert [(r["step"], r["k"]) for r in rows] == [("ok", 0), ("ok", 1), ("ok2", 0), ("ok2", 1)]
    assert all(r["forwarded"] == FORWARD for r in rows)
    assert failed == [] and finished == 2
    assert device == ["device of ok2", "1.0"]
    assert [s for s, _ in log()] == ["ok", "ok2"]


@pytest.mark.parametrize("step,status", [("bad", 3), ("killed", -9)])
def test_runner_starts_nothing_after_a_step_that_failed(fake, step, status, capsys):
    script, log = fake
    rows, failed, device, finished = probelib.run_steps(script, ["ok", step, "never"], FORWARD, 30)
    assert [(r["step"], r["k"]) for r in rows] == [("ok", 0), ("ok", 1)]  # the failed step's own row is discarded
    assert failed == [{"step": step, "status": status}] and finished == 1
    assert device == ["device of ok", "1.0"]
    assert [s for s, _ in log()] == ["ok", step]
    assert f"{step}: failed ({status}); no further step is started" in capsys.readouterr().out


def test_runner_ends_a_step_at_its_time_limit(fake):
    script, log = fake
    t0 = time.monotonic()
    rows, failed, device, finished = probelib.run_steps(script, ["ok", "slow", "never"], FORWARD, 1)
    assert time.monotonic() - t0 < 15  # a cap, not a measurement: the limit plus start-up, far below the child's 60 s
    assert [(r["step"], r["k"]) for r in rows] == [("ok", 0), ("ok", 1)]
    assert failed == [{"step": "slow", "status": "time limit"}] and finished == 1
    assert [s for s, _ in log()] == ["ok", "slow"]
    with pytest.raises(ProcessLookupError):  # the child was killed and reaped
        os.kill(int(log()[1][1]), 0)


def test_write_result_makes_the_directory(tmp_path, capsys):
    path = str(tmp_path / "deep" / "er" / "x.json")
    probelib.write_result(path, dict(rows=[1], failed=[]))
    assert json.load(open(path)) == {"rows": [1], "failed": []}
    assert capsys.readouterr().out == f"wrote {path}\n"


def test_alternate_sizes_clamps_and_alternates():
    seen = []
    # ms per call: the sizing windows first, then three rounds
    script = {"A": [0.001, 5.0, 1.0, 3.0], "B": [2.0, 20.0, 40.0, 30.0], "C": [1000.0, 7.0, 7.0, 7.0]}
    fns = {who: object() for who in script}

    def window(fn, calls):
        who = next(w for w, f in fns.items() if f is fn)
        seen.append((who, calls))
        return script[who].pop(0)

    times, calls = probelib.alternate(fns, window_ms=100.0, windows=3, first=4, lo=5, hi=2000, window=window)
    # 100 / 0.001 is above hi; 100 / 2 lies between the bounds; 100 / 1000 is below lo
    assert calls == {"A": 2000, "B": 50, "C": 5}
    assert seen == [("A", 4), ("B", 4), ("C", 4)] + [("A", 2000), ("B", 50), ("C", 5)] * 3
    assert times["A"] == dict(ms=3.0, ms_min=1.0, ms_max=5.0)
    assert times["B"] == dict(ms=30.0, ms_min=20.0, ms_max=40.0)
    assert list(times) == ["A", "B", "C"]
    # a first window that reads zero does not divide by zero: it takes the upper clamp
    assert probelib.alternate({"Z": None}, window_ms=1.0, windows=1, first=2, lo=2, hi=500, window=lambda fn, calls: 0.0)[1] == {"Z": 500}


def f32(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def test_differing_is_byte_for_byte():
    quiet_nan, payload_nan = 0x7FC00000, 0x7FC00001
    a = dict(nan=f32(quiet_nan, 0x3F800000), nan64=np.array([np.nan]), payload=f32(quiet_nan), zero=np.array([0.0], dtype=np.float32),
             kind=np.zeros(4, dtype=np.int32), shape=np.zeros((2, 3), dtype=np.float32), odd=np.array([1, 2, 3], dtype=np.uint8),
             odd_moved=np.array([1, 2, 3], dtype=np.uint8), only_a=np.zeros(1))
    b = dict(nan=f32(quiet_nan, 0x3F800000), nan64=np.array([np.nan]), payload=f32(payload_nan), zero=np.array([-0.0], dtype=np.float32),
             kind=np.zeros(4, dtype=np.float32), shape=np.zeros((3, 2), dtype=np.float32), odd=np.array([1, 2, 3], dtype=np.uint8),
             odd_moved=np.array([1, 2, 4], dtype=np.uint8), only_b=np.zeros(1))
    with pytest.raises(ValueError):  # what one of the earlier copies did to every array
        a["odd"].view(np.uint32)
    only, changed = probelib.differing(a, b)
    assert only == ["only_a", "only_b"]
    assert changed == ["kind", "odd_moved", "payload", "shape", "zero"]  # not nan, nan64 (equal bits) or odd
    assert probelib.differing(a, a) == ([], [])
    assert probelib.differing({}, {}) == ([], [])  # nothing differs in nothing: the probes must refuse that themselves (below)


def test_npz_and_directory_load_to_the_same_mapping(tmp_path):
    arrays = {"x.fwd.joints": f32(0x7FC00001, 0x80000000), "x.stats": np.arange(6, dtype=np.int64).reshape(2, 3), "sha": np.arange(3, dtype=np.uint8)}
    np.savez(tmp_path / "a.npz", **arrays)
    os.mkdir(tmp_path / "a")
    for k, v in arrays.items():
        np.save(tmp_path / "a" / f"{k}.npy", v)
    (tmp_path / "a" / "notes.txt").write_text("not an array")
    z, d = probelib.load_arrays(str(tmp_path / "a.npz")), probelib.load_arrays(str(tmp_path / "a"))
    assert sorted(z) == sorted(d) == sorted(arrays)
    assert probelib.differing(z, d) == ([], []) and probelib.differing(d, arrays) == ([], [])


@pytest.mark.parametrize("probe,as_npz", [("scan_outputs_probe.py", True), ("joints_outputs_probe.py", False), ("lbs_outputs_probe.py", False),
                                          ("raster_outputs_probe.py", False)])
def test_outputs_probes_refuse_to_compare_nothing(tmp_path, probe, as_npz):
    """``--compare`` of each of the four: equal inputs pass, one changed bit fails, and two empty inputs fail too."""
    def store(name, **arrays):
        path = str(tmp_path / (name + ".npz" if as_npz else name))
        if as_npz:
            np.savez(path, **arrays)
        else:
            os.mkdir(path)
            for k, v in arrays.items():
                np.save(os.path.join(path, k + ".npy"), v)
        return path

    def compare(a, b):
        done = subprocess.run([sys.executable, os.path.join(TOOLS, probe), "--compare", a, b], capture_output=True, text=True, timeout=60)
        return done.returncode, done.stdout + done.stderr

    full = store("full", v=np.array([0.0, np.nan], dtype=np.float32), sha=np.arange(3, dtype=np.uint8))
    same = store("same", v=np.array([0.0, np.nan], dtype=np.float32), sha=np.arange(3, dtype=np.uint8))
    moved = store("moved", v=np.array([-0.0, np.nan], dtype=np.float32), sha=np.arange(3, dtype=np.uint8))
    status, out = compare(full, same)
    assert status == 0 and "0 differ" in out, out
    status, out = compare(full, moved)
    assert status == 1 and "1 differ" in out and "DIFFERS" in out, out
    status, out = compare(store("empty_a"), store("empty_b"))
    assert status == 1 and "0 differ" in out, out
