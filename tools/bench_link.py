"""Degraded neighbour link (srb_link): what the link costs, what its kernel costs by thread mapping, and
what delay, loss and noise do to the separation of a team.

    cost     the bench team (bench.CONFIGS[3]: 1024 agents, N = 10, 3 static + 8 neighbour rows, plans on): ms per cycle
             of run(T) without a link (nominal), with a link of zero delay and zero drop (link_zero: the states, so the
             NLPs, of nominal; the difference is the link's launch and kernel alone) and with workload.link_tables and
             extrapolate (link: other NLPs from the second cycle on)
    kernel   srb_link_update_kernel alone on the same team's tables (max_delay 2, every table, plans on, extrapolate):
             microseconds per update for 1, 8 and 16 threads per row (srb_link_update_lanes_device), `reps` updates
             enqueued back to back between two device events, so a figure holds the launch gap of a stream of small
             kernels as well as the kernel
    safety   one workload.make_scenes scene of 8 agents and 20 obstacles tiled 128 times (workload.replicate_scenes,
             BatchSolver.set_scenes; 1024 agents, the replicas differ in the link's draws alone), --safety-cycles cycles (200:
             the agents of a scene share a goal and crowd there late in the rollout), bodies as in
             tools/bench_plant.py: per setting of delay (every row), drop and noise_p, one at a time, with and without
             extrapolate, the per-scene min_d_agent distribution and the collided / failed / not-converged counts.
             --cross-goals: instead of the one goal of the scene, every agent walks to the start of another agent of its
             scene (workload.cross_goals of the starts, one derangement for all replicas): paths cross and nobody shares
             a goal, the study DESIGN.md 10.14 names and 10.15 records

Method (as tools/bench_plant.py): the cost modes are warmed up, then timed in interleaved rounds -- one
run(T) per mode per round, host clock around work that ends in a device synchronise, the library's timing events off --
and the median over the rounds is reported with each mode's spread.  The kernel mappings are interleaved likewise.

    python tools/bench_link.py [--cycles 20] [--safety-cycles 200] [--rounds 7] [--reps 200] [--cross-goals] [--out FILE]

The result is printed as one JSON line and written to --out, by default profiles/bench_link.json.
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

# (delay cycles, drop, noise_p m): one factor at a time around the undegraded link
SETTINGS = ((0, 0.0, 0.0), (1, 0.0, 0.0), (2, 0.0, 0.0), (4, 0.0, 0.0), (0, 0.2, 0.0), (0, 0.5, 0.0), (0, 0.0, 0.03),
            (0, 0.0, 0.1), (2, 0.2, 0.03))
LANES = (1, 8, 16)


def spread(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def dist(v):
    v = np.asarray(v, dtype=float)
    return {"min": float(v.min()), "p05": float(np.quantile(v, 0.05)), "median": float(np.median(v)),
            "p95": float(np.quantile(v, 0.95)), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=20, help="T: cycles per rollout")
    ap.add_argument("--safety-cycles", type=int, default=200,
                    help="safety: cycles per rollout (the scene's agents share a goal: they meet there late)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1, help="untimed rollouts per mode")
    ap.add_argument("--reps", type=int, default=200, help="kernel: updates per timed window")
    ap.add_argument("--copies", type=int, default=128, help="safety: replicas of the scene")
    ap.add_argument("--team", type=int, default=8)
    ap.add_argument("--obs", type=int, default=20)
    ap.add_argument("--agents", type=int, default=0, help="cost, kernel: the team (default: the bench team's 1024)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cross-goals", action="store_true",
                    help="safety: goals exchanged within the scene (workload.cross_goals of the starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_link.json"),
                    help="the record (default: profiles/bench_link.json of this tree; '' writes none)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_link.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[3]
    N, C, T = cfg["N"], cfg["C"], args.cycles
    p = srbnmpc.default_params(N, C, K_obs=cfg["K_obs"], K_nbr=cfg["K_nbr"], use_nlp=1)
    t = lambda a, **kw: torch.as_tensor(np.ascontiguousarray(a), device=dev, **kw)

    # ---- cost: the bench team, plans on
    A = args.agents or cfg["agents"]
    _, b, _, _ = bench.rank_batch(3, A, 1, 0)
    x0, obstacles = t(b["x0"], dtype=torch.float64), t(b["obstacles"], dtype=torch.float64)
    goal = t(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    s = srbnmpc.BatchSolver(p, A, 0)
    s.set_option("timing", 0)
    delay, drop, noise_p, noise_v = workload.link_tables(A, args.seed)
    zero_link = srbnmpc.LinkModel(seed=args.seed, delay=t(np.zeros(A, np.int32)), drop=t(np.zeros(A)))
    full_link = srbnmpc.LinkModel(seed=args.seed, delay=t(delay), drop=t(drop), noise_p=t(noise_p), noise_v=t(noise_v),
                                  extrapolate=True)
    modes = [(name, srbnmpc.Rollout(s, goal, vref=workload.VREF, plans=True, obstacles=obstacles, link=link))
             for name, link in (("nominal", None), ("link_zero", zero_link), ("link", full_link))]

    def run(r, state=x0):
        r.reset(state)
        r.run(T)
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
    team_safety = {name: {"min_d_agent": float(r.results()["min_d_agent"].min().item()),
                          "min_d_obs": float(r.results()["min_d_obs"].min().item())} for name, r in modes}

    # ---- kernel: the update alone, by mapping, on the full link's buffers and the team's last truth tables
    r = modes[2][1]
    link, lib, stream = r._link(), srbnmpc.lib(), s._stream(None)
    link.age_log = None                                       # (the cycle numbers below run past the rollout's log rows)
    last, plan = srbnmpc._dptr(r.last_state), srbnmpc._dptr(r.plan_table)
    us = {lanes: [] for lanes in LANES}

    def window(lanes, c):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.reps):
            srbnmpc._check(lib.srb_link_update_lanes_device(s._h, A, ctypes.byref(link), last, plan, c + i, 0, lanes, stream))
        e1.record()
        torch.cuda.synchronize(dev)
        return 1e3 * e0.elapsed_time(e1) / args.reps
    c = 1
    for lanes in LANES:
        window(lanes, c)                                      # warm-up: the code object of every mapping
    for _ in range(args.rounds):
        for lanes in LANES:
            us[lanes].append(window(lanes, c))
            c += args.reps
    s.close()

    # ---- safety: replicas of one scene, one factor at a time
    S, sa, so = args.copies, args.team, args.obs
    A2 = S * sa
    sc = workload.replicate_scenes(workload.make_scenes(1, sa, N, C, seed=args.seed, n_obs=so), S)
    goal2, phase2, obstacles2, x02 = t(sc["goal"]), t(sc["phase"]), t(sc["obstacles"]), t(sc["x0"])
    if args.cross_goals:
        goal2 = t(workload.cross_goals(sc["nbr_state"][:, :2], sa, args.seed))
    body = t(np.full(A2, workload.FAIL_RADIUS * np.sqrt(workload.EPS_NBR) / (2 * np.sqrt(workload.EPS_OBS))))
    s2 = srbnmpc.BatchSolver(p, A2, 0)
    s2.set_option("timing", 0)
    s2.set_scenes(sa, so)
    sweep = []
    for d, q, e in SETTINGS:
        for ext in (False, True):
            if ext and d == 0 and q == 0.0:
                continue                                      # nothing ages: extrapolate changes nothing
            link = srbnmpc.LinkModel(seed=args.seed, delay=t(np.full(A2, d, np.int32)), drop=t(np.full(A2, q)),
                                     noise_p=t(np.full(A2, e)), extrapolate=ext)
            r2 = srbnmpc.Rollout(s2, goal2, vref=workload.VREF, phase=phase2, plans=True, obstacles=obstacles2,
                                 agent_body=body, link=link)
            r2.reset(x02)
            r2.run(args.safety_cycles)
            sr = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r2.scene_results().items()}
            sweep.append({"delay": d, "drop": q, "noise_p": e, "extrapolate": int(ext),
                          "agents_collided": int(sr["n_collided"].sum()), "agents_failed": int(sr["n_failed"].sum()),
                          "solves_not_converged": int(sr["n_not_converged"].sum()),
                          "scenes_with_a_collision": int((sr["n_collided"] > 0).sum()),
                          "scenes_with_a_failure": int((sr["n_failed"] > 0).sum()),
                          "max_age": int(r2.results()["link_age"].max().item()),
                          "min_d_agent": dist(sr["min_d_agent"]), "min_d_obs": dist(sr["min_d_obs"])})
    s2.close()

    res = {"tool": "tools/bench_link.py", "horizon": N, "K_obs": cfg["K_obs"], "K_nbr": cfg["K_nbr"], "cycles": T,
           "rounds": args.rounds, "n_gpus": 1, "seed": args.seed,
           "cost": {"agents": A, "plans": True, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
                    "mean_iterations_per_solve": iters, "link_zero_traj_equals_nominal": same, "team": team_safety},
           "kernel": {"agents": A, "max_delay": int(delay.max()), "updates_per_window": args.reps,
                      "us_per_update": {str(k): spread(v) for k, v in us.items()},
                      "product_lanes": "srb_link_update_device's mapping is SRB_LINK_LANES of csrc/srb_kernel_decls.h"},
           "safety": {"replicas": S, "team": sa, "obstacles_per_scene": so, "agents": A2, "cycles": args.safety_cycles,
                      "cross_goals": bool(args.cross_goals), "sweep": sweep},
           "note": "cost: run(T) / T, reset included, interleaved: nominal (no link: srb_rollout_plant_device's path), "
                   "link_zero (delay and drop tables of zeros: srb_rollout_link_device on nominal's states, the link's "
                   "launch and kernel alone), link (workload.link_tables with extrapolate: other NLPs from the second "
                   "cycle on).  kernel: microseconds per srb_link_update_lanes_device call, `updates_per_window` calls "
                   "back to back between two device events (the launch gap of a stream of small kernels is in the "
                   "figure), per threads per row.  safety: one rollout of `safety.cycles` cycles per setting, every row at the same "
                   "delay / drop / noise_p, the distribution of the per-scene min_d_agent (clearance between bodies) "
                   "over the replicas, agents collided / failed and solves not converged summed over the replicas."}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
