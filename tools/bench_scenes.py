"""Scene batching (BatchSolver.set_scenes) at the configs[2] problem shape: 128 independent teams
of 8 agents with 20 obstacles each (workload.make_scenes; N = 10, C = 2, 3 static rows + up to 8 neighbour rows,
which a team of 8 clamps to 7) on one GPU, three ways:

    scene_batched_step   one solve_device call over the 1024 agents with scenes on
    per_team_calls       the same 128 teams as 128 solve_device calls of 8 agents on one context, scenes off
    scene_rollout        Rollout.run(T) over the 1024 agents with scenes on (ms per cycle), and the fail statistics
                         of Rollout.scene_results()

and, for scale, one_team_step: the same 1024 agents solved as ONE team (scenes off: every agent selects from all
2560 obstacles and 1024 agents -- another problem, the unsegmented launch the batched one is compared with).

Method (as tools/bench_rollout.py): every mode is warmed up, then the modes are timed in interleaved rounds -- one
window per mode per round, host clock around work that ends in a device synchronise, the library's timing events
off -- and the median over the rounds is reported with each mode's spread (min, max).  Afterwards, untimed: the
selection kernel's time from the library's own events (timing on) and the metrics kernel's time from HIP events
around a loop of srb_sim_metrics_device calls, scenes on and off.

    python tools/bench_scenes.py [--scenes 128] [--team 8] [--obs 20] [--cycles 20] [--rounds 7] [--out profiles/bench_scenes.json]
"""
import argparse
import ctypes
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
    ap.add_argument("--scenes", type=int, default=128)
    ap.add_argument("--team", type=int, default=8)
    ap.add_argument("--obs", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=20, help="T: cycles per rollout window")
    ap.add_argument("--steps", type=int, default=20, help="solve steps per window of the step modes")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1, help="untimed windows per mode")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None,
                    help="diagnostics: time the variant build libsrbnmpc_<tag>.so instead of the product library")
    args = ap.parse_args()
    if args.lib:
        srbnmpc.use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_scenes.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[3]
    S, sa, so, T = args.scenes, args.team, args.obs, args.cycles
    A, N, C = S * sa, cfg["N"], cfg["C"]
    p = srbnmpc.default_params(N, C, K_obs=cfg["K_obs"], K_nbr=cfg["K_nbr"], use_nlp=1)
    b = workload.make_scenes(S, sa, N, C, seed=args.seed, n_obs=so)
    t = {k: torch.as_tensor(np.ascontiguousarray(v).reshape(v.shape[0], -1), dtype=torch.int32 if k == "phase" else torch.float64,
                            device=dev) for k, v in b.items()}
    t["phase"] = t["phase"].reshape(-1).contiguous()
    f8 = dict(dtype=torch.float64, device=dev)
    i4 = dict(dtype=torch.int32, device=dev)

    def outs(n):
        return dict(x_qp=None, x=torch.zeros((n, p.nv), **f8), obj=torch.zeros(n, **f8), status=torch.zeros((n, 2), **i4),
                    iters=torch.zeros((n, 2), **i4))

    batched = srbnmpc.BatchSolver(p, A, 0)          # scenes on
    batched.set_scenes(sa, so)
    plain = srbnmpc.BatchSolver(p, A, 0)            # scenes off: the per-team calls and the one-team step
    for s in (batched, plain):
        s.set_option("timing", 0)
    out_b, out_1, out_t = outs(A), outs(A), [outs(sa) for _ in range(S)]
    team = [{k: t[k][i * sa:(i + 1) * sa] for k in ("x0", "ref", "foot", "nbr_state")} for i in range(S)]
    team_ob = [t["obstacles"][i * so:(i + 1) * so] for i in range(S)]
    roll = srbnmpc.Rollout(batched, t["goal"], vref=workload.VREF, phase=t["phase"], obstacles=t["obstacles"])

    def scene_batched_step():
        for _ in range(args.steps):
            batched.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], out_b)

    def per_team_calls():
        for _ in range(args.steps):
            for i in range(S):
                q = team[i]
                plain.solve_device(q["x0"], q["ref"], q["foot"], team_ob[i], q["nbr_state"], out_t[i])

    def one_team_step():
        for _ in range(args.steps):
            plain.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], out_1)

    def scene_rollout():
        roll.reset(t["x0"])
        roll.run(T)

    modes = [("scene_batched_step", scene_batched_step, args.steps), ("per_team_calls", per_team_calls, args.steps),
             ("one_team_step", one_team_step, args.steps), ("scene_rollout", scene_rollout, T)]
    for _ in range(args.warmup):
        for _, f, _ in modes:
            f()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _, _ in modes}
    for _ in range(args.rounds):
        for name, f, n in modes:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            ms[name].append(1e3 * (time.perf_counter() - t0) / n)

    # the same teams, the same results: the batched step against the per-team calls (both at the automatic wave
    # count of their own batch size, so the comparison is of statuses and of x to round-off, not of bits)
    torch.cuda.synchronize(dev)
    xt = torch.cat([o["x"] for o in out_t])
    st_t = torch.cat([o["status"] for o in out_t])
    agree = {"status_equal": bool((st_t == out_b["status"]).all().item()),
             "max_abs_x_diff": float((xt - out_b["x"]).abs().max().item())}

    # untimed: the fail statistics of the scene-batched rollout
    scene_rollout()
    sr = roll.scene_results()
    torch.cuda.synchronize(dev)
    nf, nc = sr["n_failed"].cpu().numpy(), sr["n_not_converged"].cpu().numpy()
    mda, mdo = sr["min_d_agent"].cpu().numpy(), sr["min_d_obs"].cpu().numpy()
    fc = roll.results()["fail_cycle"].cpu().numpy()
    stats = {"scenes": S, "scenes_with_a_failed_agent": int((nf > 0).sum()), "failed_agents": int(nf.sum()),
             "agents_inside_0.5m_of_an_obstacle": {"at_cycle_0": int((fc == 0).sum()), "later": int((fc > 0).sum()),
                                                   "never": int((fc < 0).sum())},
             "non_converged_solves": int(nc.sum()), "solves": int(T * A),
             "scenes_with_a_non_converged_solve": int((nc > 0).sum()),
             "min_d_agent_per_scene": spread(mda), "min_d_obs_per_scene": spread(mdo)}

    # untimed: kernel times.  Selection: the library's events around the selection launch.  Metrics: HIP events
    # around a loop of metrics calls on the rollout's buffers (the state the rollout ended in).
    def knn_ms(solver, out):
        solver.set_option("timing", 1)
        v = []
        for _ in range(20):
            solver.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], out)
            solver.sync()
            v.append(solver.last_kernel_ms()[0])
        solver.set_option("timing", 0)
        return spread(v[5:])

    def metrics_ms(solver, reps=200):
        sim = roll._sim()
        lib, st = srbnmpc.lib(), solver._stream(None)
        for _ in range(10):
            srbnmpc._check(lib.srb_sim_metrics_device(solver._h, A, ctypes.byref(sim), 1, st))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            srbnmpc._check(lib.srb_sim_metrics_device(solver._h, A, ctypes.byref(sim), 1, st))
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / reps

    kernels = {"selection_ms": {"scenes": knn_ms(batched, out_b), "one_team": knn_ms(plain, out_1)},
               "metrics_ms_per_call_back_to_back": {"scenes": metrics_ms(batched), "one_team": metrics_ms(plain)},
               "note": "selection: srb_last_kernel_ms of 15 steps (srb_knn_scene_kernel / srb_knn_kernel, with its grid "
                       "build where the one-team tables are long enough); metrics: 200 back-to-back "
                       "srb_sim_metrics_device calls between two HIP events, launch overhead included"}

    res = {"tool": "tools/bench_scenes.py", "scenes": S, "team": sa, "obstacles_per_scene": so, "agents": A, "horizon": N,
           "K_obs": cfg["K_obs"], "K_nbr": cfg["K_nbr"], "K_selected": list(batched.n_selected(S * so, A)),
           "steps_per_window": args.steps, "cycles_per_window": T, "rounds": args.rounds, "n_gpus": 1,
           "ms_per_step": {k: spread(v) for k, v in ms.items()},
           "per_team_over_batched": float(np.median(ms["per_team_calls"]) / np.median(ms["scene_batched_step"])),
           "batched_equals_per_team": agree, "rollout_stats": stats, "kernels": kernels,
           "note": "ms_per_step: one solve of all 128 teams (per_team_calls: the 128 calls together); scene_rollout: ms per "
                   "cycle of Rollout.run(T), reset included.  one_team_step solves another problem (one 1024-agent team)."}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    batched.close()
    plain.close()


if __name__ == "__main__":
    main()
