"""What the probes in this directory share: the timing method, the step runner and the bit-for-bit comparison.  The probes run as
``python3 tools/x.py``, so they reach this module as ``import probelib``.  ``torch`` is imported inside the functions that need the
device: the parent of a stepped probe never opens it.

Timing (``window``, ``warm_up``, ``alternate``).  Everything is warmed up first, at every size that will be timed.  A window is as many
back-to-back calls as fill ``--window-ms`` between two device events, ended by a synchronise; the number of calls is sized from a
first short window of ``first`` calls and clamped to ``lo`` .. ``hi`` (each probe states its three numbers).  The windows of the
variants ALTERNATE, ``--windows`` of each, so that a drift of the machine falls on all of them alike, and the median and the spread
(min, max) of the per-call time are recorded.  The times are those of the whole Python call - argument checks, output allocation,
autograd bookkeeping and launch latency included.

Steps (``run_steps`` in the parent; ``emit_row``, ``emit_device`` in the child).  A stepped probe runs every step as a child process
of its own (``--step NAME``) under its own time limit, so a step that hangs or faults ends alone, and after a step that failed it
starts no other: on a shared machine nothing more is started on a device that has just faulted.  What a failed step printed is
discarded.

Comparison (``load_arrays``, ``differing``).  Two sets of named arrays are equal when they hold the same names and every pair agrees
in dtype, shape and raw bytes, which holds for every dtype and lets NaNs compare.  A probe's stated exceptions apply only to names
that ``differing`` returned, and a comparison of nothing is a failure.
"""
import json
import os
import statistics
import subprocess
import sys

import numpy as np


def window(fn, calls):
    """ms per call over ``calls`` back-to-back calls"""
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / calls


def warm_up(fns, n):
    import torch

    for fn in fns:
        for _ in range(n):
            fn()
    torch.cuda.synchronize()


def alternate(variants, *, window_ms, windows, first, lo, hi, window=window):
    """``variants``: who -> fn, in the order their windows take turns.  Returns (times, calls): per who ``dict(ms, ms_min, ms_max)``, the
    median and the spread of the per-call time over its windows, and the calls one of its windows held.  ``window`` is a parameter
    for the test only."""
    calls = {who: int(min(hi, max(lo, window_ms / max(window(fn, first), 1e-6)))) for who, fn in variants.items()}
    seen = {who: [] for who in variants}
    for _ in range(windows):
        for who, fn in variants.items():
            seen[who].append(window(fn, calls[who]))
    return {who: dict(ms=statistics.median(t), ms_min=min(t), ms_max=max(t)) for who, t in seen.items()}, calls


def emit_row(row):
    print("ROW " + json.dumps(row), flush=True)


def emit_device(payload):
    print("DEVICE " + json.dumps(payload), flush=True)


def run_steps(script, steps, forward, step_seconds):
    """Runs ``script --step STEP *forward`` for every step in turn, until one fails.  Returns (rows, failed, device, finished): the rows
    of the steps that finished (printed as they are read), ``[dict(step, status)]`` of the one that did not (its return code, or
    "time limit"), the last DEVICE payload, and the number of steps that finished."""
    rows, failed, device, finished = [], [], None, 0
    for step in steps:
        try:
            done = subprocess.run([sys.executable, script, "--step", step, *forward], capture_output=True, text=True, timeout=step_seconds)
            status, out = done.returncode, done.stdout
            if status != 0:
                sys.stderr.write(done.stderr[-2000:])
        except subprocess.TimeoutExpired:  # (subprocess.run has killed and reaped the child)
            status, out = "time limit", ""
        if status != 0:
            failed.append(dict(step=step, status=status))
            print(f"{step}: failed ({status}); no further step is started", flush=True)
            break
        for line in out.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
            elif line.startswith("DEVICE "):
                device = json.loads(line[7:])
        finished += 1
    return rows, failed, device, finished


def write_result(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {path}")


def load_arrays(path):
    """name -> array of a .npz, or of a directory of .npy files (memory-mapped: a directory may hold gigabytes)"""
    if os.path.isdir(path):
        return {n[:-4]: np.load(os.path.join(path, n), mmap_mode="r") for n in sorted(os.listdir(path)) if n.endswith(".npy")}
    return dict(np.load(path))


def differing(a, b):
    """(names in only one of the two, names whose dtype, shape or bytes differ), both sorted"""
    changed = []
    for n in sorted(set(a) & set(b)):
        x, y = a[n], b[n]
        if not (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()):
            changed.append(n)
    return sorted(set(a) ^ set(b)), changed
