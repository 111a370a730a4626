"""Cost of a principal-point table on the fit iteration: one bench.py workload (default cfg3, the multi-view one) timed with the
centred cameras and with a per-view principal table installed through ``SMALFitter.set_cameras``, in one process, alternating,
so that both see the same machine state.  Prints one JSON line.

    python tools/pinhole_probe.py --workload cfg3 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the workload table)
from smilify_amd import model_io, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--offset", type=float, default=0.05, help="largest |px|, |py| of the table (NDC)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[args.workload]
    tables = model_io.load_model(os.path.join(REPO, "data", "models", wl["model"] + ".npz"))
    frames, views, S = (args.frames or wl["frames"]), wl["views"], wl["S"]
    pp = args.offset * (2.0 * torch.rand(views, 2, generator=torch.Generator().manual_seed(1)) - 1.0)

    def make(principal):
        f = synthetic.make_problem(tables, frames, views, S, dev, radius=wl["radius"], seed=1234, window=10)
        if principal is not None:
            f.set_cameras(f.renderer.cameras.R, f.renderer.cameras.T, principal_point=principal)
        f.begin_stage(synthetic.STAGE1_LR, fov_lr=1.0)
        for _ in range(args.warmup):
            f.fit_step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL, window=10)
        return f

    fitters = {"centred": make(None), "principal": make(pp)}
    ms = {k: [] for k in fitters}
    for _ in range(args.rounds):
        for k, f in fitters.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f.fit_step(synthetic.STAGE1_WEIGHTS, synthetic.STAGE1_TEMPORAL, window=10)
            torch.cuda.synchronize()
            ms[k].append(1000.0 * (time.perf_counter() - t0) / args.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps(dict(workload=args.workload, frames=frames, views=views, S=S, steps=args.steps, rounds=args.rounds, offset=args.offset,
                          ms_per_step=ms, median_ms=med, principal_over_centred=med["principal"] / med["centred"])))


if __name__ == "__main__":
    main()
