"""Agent sizes (srb_agent_sizes): what the agent tables and the neighbour clearance selection cost.

    step       one solve_device call on the configs[2] batch (1024 agents, N = 10, C = 2, 3 static + 8 neighbour rows):
               without a table, with a velocity table only (the _mv_ instance and nothing else), with agent_rad, with
               agent_pad, with both, with both and the neighbour clearance selection
    selection  one select_device call (both tables) on the same batch: the snapshot selection (srb_knn_kernel, whose
               neighbour half at n_all = 1024 is its thresholded scan of rows held in registers, no grid) against the
               brute-force clearance scan (srb_knn_nbr_clear_kernel)

The step modes with a table solve different NLPs from the mode without (other levels, other selected rows, so other
iteration counts): their difference is not the cost of the code.  The cost of the code is vel_only against the parent
build's same call (profiles/agents_ab.txt) and the two selection modes against each other.

Method (as tools/bench_sizes.py): every mode is warmed up, then the modes are timed in interleaved rounds -- one
window per mode per round, host clock around work that ends in a device synchronise, the library's timing events
off -- and the median over the rounds is reported with each mode's spread (min, max).  The tables are
workload.agent_sizes(n_all, seed).

    python tools/bench_agents.py [--steps 20] [--rounds 7] [--out FILE]

The result is printed as one JSON line and written to --out, by default profiles/bench_agents.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "srb-cbf-nmpc_amd")]
import bench  # noqa: E402
import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1, help="untimed windows per mode")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_agents.json"),
                    help="the record (default: profiles/bench_agents.json of this tree; '' writes none)")
    ap.add_argument("--lib", default=None,
                    help="diagnostics: time the variant build libsrbnmpc_<tag>.so instead of the product library")
    args = ap.parse_args()
    if args.lib:
        srbnmpc.use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_agents.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[3]
    N, C, A = cfg["N"], cfg["C"], cfg["agents"]
    p = srbnmpc.default_params(N, C, K_obs=cfg["K_obs"], K_nbr=cfg["K_nbr"], use_nlp=1)
    f8 = dict(dtype=torch.float64, device=dev)
    i4 = dict(dtype=torch.int32, device=dev)
    t = {k: torch.as_tensor(np.ascontiguousarray(v).reshape(v.shape[0], -1), **f8)
         for k, v in workload.make_batch(A, N, C, seed=args.seed).items()}
    n_obs = int(t["obstacles"].shape[0])
    rad, pad, _ = (torch.as_tensor(v, device=dev) for v in workload.agent_sizes(A, args.seed))
    vel = torch.as_tensor(workload.obstacle_velocities(n_obs, args.seed), device=dev)
    s = srbnmpc.BatchSolver(p, A, 0)
    s.set_option("timing", 0)
    out = dict(x_qp=None, x=torch.zeros((A, p.nv), **f8), obj=torch.zeros(A, **f8), status=torch.zeros((A, 2), **i4),
               iters=torch.zeros((A, 2), **i4))
    sel = torch.zeros((A, sum(s.n_selected(n_obs, A))), **i4)
    bad = {}

    def step(name, **kw):
        def f():
            for _ in range(args.steps):
                s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], out, **kw)
        return name, f

    def select(name, **kw):
        def f():
            for _ in range(args.steps):
                s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, **kw)
        return name, f

    modes = [step("step_off"), step("step_vel_only", obs_vel=vel), step("step_rad", agent_rad=rad),
             step("step_pad", agent_pad=pad), step("step_rad_pad", agent_rad=rad, agent_pad=pad),
             step("step_rad_pad_clearance", agent_rad=rad, agent_pad=pad, nbr_clearance=True),
             select("select_off"), select("select_clearance", agent_rad=rad, nbr_clearance=True)]
    for _ in range(args.warmup):
        for _, f in modes:
            f()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _ in modes}
    for _ in range(args.rounds):
        for name, f in modes:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    for name, f in modes:                    # after the timing: the solves of each step mode that did not converge
        if name.startswith("step_"):
            f()
            st = out["status"]
            bad[name] = int((~(((st[:, 0] == 0) | (st[:, 0] == 4)) & (st[:, 1] == 0))).sum())
    res = {"tool": "tools/bench_agents.py", "horizon": N, "K_obs": cfg["K_obs"], "K_nbr": cfg["K_nbr"],
           "batch": {"agents": A, "obstacles": n_obs}, "calls_per_window": args.steps, "rounds": args.rounds, "n_gpus": 1,
           "ms_per_call": {k: spread(v) for k, v in ms.items()},
           "non_converged_solves_last_step": bad,
           "note": "step_*: ms per solve_device call (selection + solve) of the configs[2] batch; select_*: ms per "
                   "select_device call (both tables).  off: no table; vel_only: a velocity table alone (the _mv_ "
                   "instance, the NLP of moving obstacles); rad / pad / rad_pad: the agent tables (the selection is then "
                   "the one of off); clearance: nbr_clearance=True (the neighbour columns by srb_knn_nbr_clear_kernel, "
                   "brute force over the 1024 rows, the static columns by srb_knn_kernel).  The step modes solve "
                   "different NLPs: their differences are not code cost."}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    s.close()


if __name__ == "__main__":
    main()
