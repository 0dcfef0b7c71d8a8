"""Cost of the plan-coupled step at the configs[2] shape (1024 agents, N = 10, 3 static + 8 neighbour rows,
bench.py --config 3's batch) on one GPU: a plain solve_device step against solve_coupled_device at outer =
1, 2, 3, each with the snapshot (plan_selection 0) and the horizon-aware (1) neighbour selection, and the
neighbour-selection kernels alone.

Method (as bench.py): every mode is warmed up, then the modes are timed in interleaved rounds -- one window
of --steps steps per mode per round, host clock around work that ends in a device synchronise, the library's
own timing events off -- and the median over the rounds is reported with the spread (min, max) of each mode,
so a difference between two modes can be read against the spread of one.  plan_selection 0 starts round 0
from the constant-velocity rows (nbr_plan None: the plain step's problem); plan_selection 1 needs a table
for round 0 and takes the previous cycle's plans (a plain solve's, shifted by one grid: dist.shift_plans).
plan_change and the share of non-OPTIMAL results per round come from one untimed coupled solve per outer.

    python tools/bench_coupled.py [--steps 30] [--rounds 7] [--out profiles/NAME.json]
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
from srbnmpc import dist as sdist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agents", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_coupled.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[3]
    A = args.agents or cfg["agents"]
    N, C = cfg["N"], cfg["C"]
    p = srbnmpc.default_params(N, C, K_obs=cfg["K_obs"], K_nbr=cfg["K_nbr"], use_nlp=1)
    _, b, _, _ = bench.rank_batch(3, A, 1, 0)
    t = {k: torch.as_tensor(np.ascontiguousarray(v).reshape(v.shape[0], -1), dtype=torch.float64, device=dev)
         for k, v in b.items()}
    out = dict(x_qp=None, x=torch.zeros((A, p.nv), dtype=torch.float64, device=dev),
               obj=torch.zeros(A, dtype=torch.float64, device=dev),
               status=torch.zeros((A, 2), dtype=torch.int32, device=dev),
               iters=torch.zeros((A, 2), dtype=torch.int32, device=dev),
               plan=torch.zeros((A, N, 2), dtype=torch.float64, device=dev))
    plain_out = {k: v for k, v in out.items() if k != "plan"}
    solver = srbnmpc.BatchSolver(p, A, 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    Ko, Kn = solver.n_selected(t["obstacles"].shape[0], A)
    sel = torch.zeros((A, Ko + Kn), dtype=torch.int32, device=dev)
    args_ = (t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"])

    # the previous cycle's plans, shifted by one grid: round 0's table of the plan_selection = 1 modes
    solver.solve_device(*args_, out, stream=stream.cuda_stream, obstacles_version=1)
    prev = sdist.shift_plans(out["plan"], 1).contiguous()
    torch.cuda.synchronize(dev)

    def plain():
        solver.solve_device(*args_, plain_out, stream=stream.cuda_stream, obstacles_version=1)

    def coupled(outer, ps):
        def f():
            return solver.solve_coupled_device(*args_, out, outer=outer, nbr_plan=prev if ps else None,
                                               stream=stream.cuda_stream, obstacles_version=1)
        return f

    def select(ps):
        def f():
            solver.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, tables=2, stream=stream.cuda_stream,
                                 nbr_plan=prev if ps else None)
        return f

    modes = [("plain", 0, plain)]
    for ps in (0, 1):
        for outer in (1, 2, 3):
            modes.append((f"coupled_outer{outer}_sel{ps}", ps, coupled(outer, ps)))
    for ps in (0, 1):
        modes.append((f"select_neighbours_sel{ps}", ps, select(ps)))

    def run(ps, f, n):
        solver.set_option("plan_selection", ps)
        for _ in range(n):
            f()

    # untimed: plan_change and statuses per outer count
    rounds_info = {}
    for ps in (0, 1):
        for outer in (1, 2, 3):
            solver.set_option("plan_selection", ps)
            ch = coupled(outer, ps)()
            torch.cuda.synchronize(dev)
            st = out["status"].cpu().numpy()
            rounds_info[f"outer{outer}_sel{ps}"] = {
                "plan_change": [float(v) for v in ch.cpu().tolist()],
                "non_optimal_frac_last_round": float(1.0 - (np.isin(st[:, 0], (0, 4)) & (st[:, 1] == 0)).mean())}
    solver.set_option("timing", 0)
    for _, ps, f in modes:
        run(ps, f, args.warmup)
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _, _ in modes}
    for _ in range(args.rounds):
        for name, ps, f in modes:
            n = args.steps * (10 if name.startswith("select") else 1)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(ps, f, n)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    solver.set_option("plan_selection", 0)
    res = {"tool": "tools/bench_coupled.py", "agents": A, "horizon": N, "K_obs": cfg["K_obs"], "K_nbr": cfg["K_nbr"],
           "steps_per_window": args.steps, "rounds": args.rounds, "n_gpus": 1,
           "ms_per_step": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                           for k, v in ms.items()},
           "note": "select_neighbours_*: srb_select_device(tables = 2) alone, launch included (host clock over 10x "
                   "the steps); sel0 srb_knn_kernel on the snapshot, sel1 srb_knn_plan_kernel",
           "rounds_info": rounds_info}
    pl = res["ms_per_step"]["plain"]
    res["outer1_vs_plain"] = {"plain_spread_ms": pl["max"] - pl["min"],
                              "outer1_minus_plain_ms": res["ms_per_step"]["coupled_outer1_sel0"]["median"] - pl["median"]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    solver.close()


if __name__ == "__main__":
    main()
