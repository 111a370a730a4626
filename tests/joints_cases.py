"""The models and cases tests/test_joints_cpu.py and tests/test_gpu_joints.py share for the mesh-free joints path
(smilify_amd/joints.py, smilify_amd/csrc/joints.hip).  A case is a ``lbs_ref64.make_case`` whose vertex probe is replaced by zeros:
the objective is ``sum(joints * probe)`` alone, and ``lbs_ref64.reference`` (dense LBS over every vertex, float64) is the truth.
Holds no kernels and touches no GPU."""
import functools

import numpy as np
import torch

import lbs_cases
import lbs_ref64
from smilify_amd import model_io
from smilify_amd.joints import JointTables


@functools.lru_cache(maxsize=None)
def _random(wide):
    """The first seeded ``lbs_cases.random_model`` that regresses its joints from the vertices, has shape directions and - not
    ``wide`` - a joint that regresses from more than 4 bones; ``wide``: more than 128 joints (NJ >= 3 in the kernels)."""
    for seed in range(400):
        t = lbs_cases.random_model(np.random.default_rng(7000 + seed), wide=wide)
        if t.static_joints or t.nB < 3 or t.V > 2500:
            continue
        if wide and t.J <= 128:
            continue
        if not wide and int(np.diff(JointTables.from_tables(t).pair_ptr).max()) <= 4:
            continue
        return t
    raise AssertionError("no seeded random model meets the conditions")


@functools.lru_cache(maxsize=None)
def _synthetic(J, side, nB, static):
    return model_io.synthetic_model(V_side=side, J=J, nB=nB, seed=5, static_joints=static)


def get_model(key, tables):
    """``key``: a name of the ``tables`` fixture (stick, mouse, synthetic, synthetic_static), ``j3`` / ``j64`` / ``j65`` (procedural
    tubes of that many joints), ``j65_static``, ``random`` or ``random_wide``."""
    if key in ("random", "random_wide"):
        return _random(key == "random_wide")
    if key.startswith("j"):
        return _synthetic(int(key[1:].split("_")[0]), 6, 3, key.endswith("_static"))
    return tables(key)


def joints_case(t, **kw):
    """A ``make_case`` without a vertex objective."""
    kw = dict(kw)
    if isinstance(kw.get("theta"), str):
        kw["theta"] = lbs_ref64.edge_theta(t.J, kw["seed"])
    case = lbs_ref64.make_case(t, **kw)
    case["up"]["d_verts"] = torch.zeros_like(case["up"]["d_verts"])
    return case
