"""Disturbed plant (srb_plant): a Monte-Carlo over disturbances of one scene, and what the plant costs.

One workload.make_scenes scene of 8 agents and 20 obstacles (N = 10, C = 2, the configs[2] rows: 3 static + up to 8
neighbour rows, so here the 7 team mates) is tiled 128 times with workload.replicate_scenes and rolled out for T = 20
cycles in one launch per cycle (BatchSolver.set_scenes).  The replicas share the start configuration and differ in
their kicks alone, because they differ in their global rows.

    safety   per kick_v bound of the sweep (zero included): n_failed, n_collided and n_not_converged per scene, and
             the distribution of the per-scene min_d_obs / min_d_agent (Rollout.scene_results()).  Bodies: every agent
             0.5 sqrt(eps_nbr) / (2 sqrt(eps_obs)) m, the reference's ratio of fail radius to safety radius applied to
             half the inter-agent safety distance; d_agent is then the clearance between bodies.
    cost     ms per cycle of run(T) without the plant (nominal), with zero kick tables and one zero push per scene
             (plant_zero: the states, so the NLPs, of nominal; the difference is the plant's code alone), with the
             model's own height as plant_hcom besides (plant_zero_hcom: states within round-off of nominal's), and
             with every drawn table and one 0.22 m/s push per scene (plant: other NLPs)

Method (as tools/bench_scenes.py): both cost modes are warmed up, then timed in interleaved rounds --
one run(T) per mode per round, host clock around work that ends in a device synchronise, the library's timing events
off -- and the median over the rounds is reported with each mode's spread (min, max).  The plant mode solves other
NLPs than nominal from the second cycle on (the disturbed states differ), so its difference is the plant's code plus
whatever the disturbed problems cost the solver; the code alone is plant_zero against nominal.

    python tools/bench_plant.py [--copies 128] [--cycles 20] [--rounds 7] [--out FILE]

The result is printed as one JSON line and written to --out, by default profiles/bench_plant.json.
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

KICKS = (0.0, 0.02, 0.05, 0.1, 0.2)      # kick_v bounds (m/s per cycle): none, 7 %, 19 %, 37 %, 74 % of VREF


def spread(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def dist(v):
    v = np.asarray(v, dtype=float)
    return {"min": float(v.min()), "p05": float(np.quantile(v, 0.05)), "median": float(np.median(v)),
            "p95": float(np.quantile(v, 0.95)), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=128, help="replicas of the scene")
    ap.add_argument("--team", type=int, default=8)
    ap.add_argument("--obs", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=20, help="T: cycles per rollout")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rollouts per mode")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_plant.json"),
                    help="the record (default: profiles/bench_plant.json of this tree; '' writes none)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plant.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[3]
    N, C, S, sa, so, T = cfg["N"], cfg["C"], args.copies, args.team, args.obs, args.cycles
    A = S * sa
    p = srbnmpc.default_params(N, C, K_obs=cfg["K_obs"], K_nbr=cfg["K_nbr"], use_nlp=1)
    sc = workload.replicate_scenes(workload.make_scenes(1, sa, N, C, seed=args.seed, n_obs=so), S)
    t = lambda a, **kw: torch.as_tensor(np.ascontiguousarray(a), device=dev, **kw)
    goal, phase, obstacles, x0 = t(sc["goal"]), t(sc["phase"]), t(sc["obstacles"]), t(sc["x0"])
    body = t(np.full(A, workload.FAIL_RADIUS * np.sqrt(workload.EPS_NBR) / (2 * np.sqrt(workload.EPS_OBS))))
    s = srbnmpc.BatchSolver(p, A, 0)
    s.set_option("timing", 0)
    s.set_scenes(sa, so)

    def rollout(**plant):
        return srbnmpc.Rollout(s, goal, phase=phase, obstacles=obstacles, agent_body=body, **plant)

    def run(r):
        r.reset(x0)
        r.run(T)

    # ---- safety: the sweep over kick_v bounds
    sweep = []
    for kick in KICKS:
        r = rollout(kick_v=t(np.full(A, kick)), plant_seed=args.seed)
        run(r)
        sr = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.scene_results().items()}
        sweep.append({"kick_v": kick, "n_failed": sr["n_failed"].tolist(), "n_collided": sr["n_collided"].tolist(),
                      "n_not_converged": sr["n_not_converged"].tolist(),
                      "scenes_with_a_failure": int((sr["n_failed"] > 0).sum()),
                      "scenes_with_a_collision": int((sr["n_collided"] > 0).sum()),
                      "min_d_obs": dist(sr["min_d_obs"]), "min_d_agent": dist(sr["min_d_agent"])})

    # ---- cost: interleaved
    kv, kp, hc = (t(v) for v in workload.plant_tables(A, args.seed))
    zero, hmodel = t(np.zeros(A)), t(np.full(A, p.hcom))
    when, who = t(np.full(S, T // 2, np.int32)), t((sa * np.arange(S)).astype(np.int32))
    pushes, pushes0 = (when, who, t(np.tile([0.2, 0.1], (S, 1)))), (when, who, t(np.zeros((S, 2))))
    modes = [("nominal", rollout()),
             ("plant_zero", rollout(kick_v=zero, kick_p=zero, pushes=pushes0, plant_seed=args.seed)),
             ("plant_zero_hcom", rollout(kick_v=zero, kick_p=zero, plant_hcom=hmodel, pushes=pushes0,
                                         plant_seed=args.seed)),
             ("plant", rollout(kick_v=kv, kick_p=kp, plant_hcom=hc, pushes=pushes, plant_seed=args.seed))]
    for _ in range(args.warmup):
        for _, r in modes:
            run(r)
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _ in modes}
    for _ in range(args.rounds):
        for name, r in modes:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(r)
            torch.cuda.synchronize(dev)
            ms[name].append(1e3 * (time.perf_counter() - t0) / T)
    iters = {name: float(r.results()["iters"].double().sum(2).mean().item()) for name, r in modes}
    same = bool(torch.equal(modes[0][1].results()["traj"], modes[1][1].results()["traj"]))
    res = {"tool": "tools/bench_plant.py", "horizon": N, "K_obs": cfg["K_obs"], "K_nbr": cfg["K_nbr"],
           "batch": {"replicas": S, "team": sa, "obstacles_per_scene": so, "agents": A}, "cycles": T,
           "rounds": args.rounds, "n_gpus": 1, "seed": args.seed, "sweep": sweep,
           "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
           "mean_iterations_per_solve": iters, "plant_zero_traj_equals_nominal": same,
           "note": "sweep: one rollout of T cycles per kick_v bound (kick_v alone, uniform over the agents), the "
                   "per-scene lists in replica order and the distribution of the per-scene minima over the replicas; "
                   "min_d_agent is the clearance between bodies.  ms_per_cycle: run(T) / T, reset included, interleaved: "
                   "nominal (no plant argument: srb_rollout_agents_device); plant_zero (zero kick_v and kick_p, one "
                   "zero push per scene at cycle T / 2: srb_rollout_plant_device on nominal's states, the plant's "
                   "code alone); plant_zero_hcom (plant_hcom = the model's besides); plant (kick_v, kick_p, "
                   "plant_hcom of workload.plant_tables and one (0.2, 0.1) m/s push per scene: other NLPs from the "
                   "second cycle on).  mean_iterations_per_solve: QP + NLP iterations per agent and cycle."}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    s.close()


if __name__ == "__main__":
    main()
