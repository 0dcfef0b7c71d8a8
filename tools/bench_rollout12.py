"""Closed-loop rollout of the SRB-12 mode at the shape of bench.py --path srb12 (1024 agents, N = 10, trot, 3 static
+ 8 neighbour rows, workload.make_batch12 seed 1234) on one GPU: cycles per second of the C driver
(Rollout12.run(T): advance, metrics and solve enqueued from one call), of T x Rollout12.step() from Python, of the
plain solve_device loop that re-solves the same inputs (no advance, no metrics, no state carried), and of a
scene-batched rollout (128 scenes x 8 agents x 20 obstacles, workload.make_scenes12); the advance and metrics
kernels alone, next to the LIP mode's advance at the same agent count; and the separation the team keeps.

Method (as tools/bench_rollout.py): every mode is warmed up, then the modes are timed in interleaved rounds -- one
window of T cycles per mode per round, host clock around work that ends in a device synchronise, the library's
timing events off -- and the median over the rounds is reported with each mode's spread (min, max).  Every window of
a rollout mode starts from the same reset state and runs the same T cycles.  The kernels alone are timed the same
way, a window being T back-to-back calls at cycle 1 (the later-cycle path, with the logs).

    python tools/bench_rollout12.py [--cycles 20] [--rounds 7] [--out profiles/bench_rollout12.json]

--plans adds the neighbour plans (srb12_plans) next to the modes above, in the same interleaved
rounds: Rollout12(plans=True).run(T), T x step() and the scene-batched run, with and without the horizon-aware
selection; the shift kernel alone; the selection alone, snapshot and horizon-aware (the library's timing events on a
context of its own); the separation with the plans on beside the plans-off rollout of the same run; and plan_change
per Jacobi round of Solver12.solve_coupled_device on the 1024-agent batch.

    python tools/bench_rollout12.py --plans --out profiles/bench_rollout12_plans.json

--moving measures the moving obstacles instead (srb_moving), by the same method: the rollout cycle
(Rollout12.run(T), reset included) with the velocity table off / on / on with the horizon-aware obstacle selection,
for the 1024-agent team and for the 128 x 8 scene batch; and the separation table of 10.6 over T cycles of the moved
world (velocities workload.obstacle_velocities(n_obs, 1234, --vmax)): the solver aware of the velocities, with and
without the horizon selection, against obs_vel=None -- a solver that re-reads the moved table every cycle and takes it
for static.

    python tools/bench_rollout12.py --moving [--vmax 1.0] [--out profiles/bench_rollout12_moving.json]

--sizes measures the obstacle sizes instead (srb_sizes), by the same method: the rollout cycle
(Rollout12.run(T), reset included) without a table, with obs_eps, and with obs_eps + obs_clearance, each with and
without obs_radius (tables workload.obstacle_sizes(n_obs, 1234)), for the 1024-agent team and for the 128 x 8 scene
batch; and the separation table of 10.7's form over T cycles: the smallest and the median clearance to the obstacle
bodies, the agents inside a body and the non-converged solves of the three solves (all measured with obs_radius).
The three solves are three different NLPs -- other levels, other rows -- so their times have no target.

    python tools/bench_rollout12.py --sizes [--out profiles/bench_rollout12_sizes.json]

--agents (without a number; --agent-sizes is the same switch) measures the agent sizes instead (srb_agent_sizes,
DESIGN.md 10.11), the rows of the --sizes table with the agent tables: the rollout cycle without a table, with
agent_rad + agent_pad, and with those + nbr_clearance, each with and without agent_body (tables
workload.agent_sizes(n_all, 1234)), for the 1024-agent team and for the 128 x 8 scene batch; and the separation over T
cycles: the smallest and the median clearance between bodies, the agents that touched another body and the
non-converged solves of the three solves (all measured with agent_body).  Three different NLPs again: no target.

    python tools/bench_rollout12.py --agents [--out profiles/bench_rollout12_agents.json]

--plant measures the disturbed plant instead (srb12_plant): one workload.make_scenes12 scene (8 agents,
20 obstacles, seed 1234) tiled by workload.replicate_scenes to --agents agents under set_scenes(8, 20), T cycles by
run().  Cost, by the method above (Rollout12.run(T), reset included): nominal (the parent's path); the plant with zero
bounds and one zero push per scene; that with mass = the model's, which runs the roll; that with at_state; and the drawn
tables of workload.plant_tables12 with one push per scene.  The tool checks that the zero rows reproduce the nominal
traj: bit for bit without a roll, within the polish's dynamics tolerance carried over the rollout with one (at_state
is another plant: its departure is reported, not checked).  Safety: the sweep over kick_v bounds of 10.12.
Linearisation: with no kicks, at_state 1 against 0 -- the largest departure of the plant from the prediction,
min_d_obs and the scenes with a failure.

    python tools/bench_rollout12.py --plant [--out profiles/bench_rollout12_plant.json]

--link measures the degraded neighbour link instead (srb_link on an SRB-12 context), with the protocol
of tools/bench_link.py (10.14).  Cost, on the bench team above with plans on (Rollout12.run(T), reset included,
interleaved rounds): nominal (no link: srb12_rollout_plant_device's path); link_zero (delay and drop tables of zeros:
the link's launch and kernel on nominal's states, whose traj the tool checks to be the nominal one's); link
(workload.link_tables with extrapolate); and nominal and link once more with the horizon-aware selection, whose own plan
the link run takes from the truth.  Safety: one workload.make_scenes12 scene (8 agents, 20 obstacles, seed 1234) tiled to
--agents agents under set_scenes(8, 20), bodies as in tools/bench_link.py, --safety-cycles cycles per rollout, the
settings of tools/bench_link.py one factor at a time, each with and without extrapolate and with and without
plan_selection, once per K_nbr of --safety-knbr (default 8 and 3).  --cross-goals: every agent walks to the start of another agent of its scene (workload.cross_goals)
instead of to the scene's one goal.

    python tools/bench_rollout12.py --link --cross-goals [--safety-cycles 200] [--out profiles/bench_rollout12_link.json]
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
import srbnmpc  # noqa: E402
from srbnmpc import srb12, workload  # noqa: E402

EDGES = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 1e9]


def hist(v):
    v = np.asarray(v)
    return {"edges_m": EDGES[:-1] + ["inf"], "counts": [int(c) for c in np.histogram(v, EDGES)[0]],
            "min": float(v.min()), "median": float(np.median(v)), "max": float(v.max())}


def safety_of(r):
    st = r["status"].cpu().numpy()
    fc = r["fail_cycle"].cpu().numpy()
    z = r["traj"][:, :, 2].cpu().numpy()
    return {"min_d_agent": hist(r["min_d_agent"].cpu().numpy()), "min_d_obs": hist(r["min_d_obs"].cpu().numpy()),
            "agents_inside_0.5m_of_an_obstacle": {"at_cycle_0": int((fc == 0).sum()), "later": int((fc > 0).sum()),
                                                  "never": int((fc < 0).sum())},
            "height_m": {"min": float(z.min()), "max": float(z.max())},
            "non_optimal_frac_per_cycle": [float(1.0 - (np.isin(s[:, 0], (0, 4)) & (s[:, 1] == 0)).mean()) for s in st]}


def moving(args):
    """--moving: see the module docstring."""
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs = 8, 20
    S = A // team
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    b = workload.make_batch12(A, N, "trot", seed=1234)
    sb = workload.make_scenes12(S, team, N, "trot", seed=1234, n_obs=scene_obs)
    goal = D(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    worlds = {}
    for name, x0, g, phase, ob, scenes in (("one_team", b["x0"], goal, None, b["obstacles"], (0, 0)),
                                           ("scenes", sb["x0"], D(sb["goal"]), D(sb["phase"], torch.int32), sb["obstacles"],
                                            (team, scene_obs))):
        solver = srb12.Solver12(p, x0.shape[0], 0)
        solver.set_timing(False)
        solver.set_scenes(*scenes)
        ob = D(ob)
        vel = D(workload.obstacle_velocities(ob.shape[0], 1234, args.vmax))
        mk = lambda v, h: srb12.Rollout12(solver, g, vref=workload.VREF, phase=phase, obstacles=ob, obs_vel=v, obs_horizon=h)
        worlds[name] = dict(solver=solver, x0=D(x0), ob=ob, vel=vel, goal=g, phase=phase,
                            rolls={"off": mk(None, False), "on": mk(vel, False), "on_horizon": mk(vel, True)})

    def cycle(w, r):
        def f():
            r.reset(w["x0"])
            r.run(T)
        return f
    modes = [(f"{name}_{k}", cycle(w, r)) for name, w in worlds.items() for k, r in w["rolls"].items()]
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
            ms[name].append(1e3 * (time.perf_counter() - t0) / T)

    def stats(r):
        res = r.results()
        torch.cuda.synchronize(dev)
        d, fc, st = res["min_d_obs"].cpu().numpy(), res["fail_cycle"].cpu().numpy(), res["status"].cpu().numpy()
        ok = np.isin(st[..., 0], (0, 4)) & (st[..., 1] == 0)
        return {"min_d_obs": {"smallest": float(d.min()), "median": float(np.median(d))},
                "agents_inside_0.5m": {"at_cycle_0": int((fc == 0).sum()), "later": int((fc > 0).sum()),
                                       "never": int((fc < 0).sum())},
                "non_converged_solves": int((~ok).sum()), "solves": int(ok.size)}
    sep = {}
    for name, w in worlds.items():
        sep[name] = {}
        for k, label in (("on", "aware"), ("on_horizon", "aware_horizon_selection")):
            cycle(w, w["rolls"][k])()
            sep[name][label] = stats(w["rolls"][k])
        table = w["ob"].clone()                       # the unaware solver: the table moves, the solver is not told
        blind = srb12.Rollout12(w["solver"], w["goal"], vref=workload.VREF, phase=w["phase"], obstacles=table)
        blind.reset(w["x0"])
        for c in range(T):
            if c > 0:
                w["solver"].advance_obstacles_device(table, w["vel"])
            blind.step()
        sep[name]["obs_vel_none"] = stats(blind)
    spread = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res = {"tool": "tools/bench_rollout12.py --moving", "agents": A, "horizon": N, "K_obs": Ko, "K_nbr": Kn,
           "vmax": args.vmax, "scenes": {"n_scenes": S, "scene_agents": team, "scene_obs": scene_obs},
           "one_team_obstacles": int(worlds["one_team"]["ob"].shape[0]), "cycles_per_window": T, "rounds": args.rounds,
           "n_gpus": 1, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
           "separation_over_cycles": T, "separation": sep,
           "note": "ms_per_cycle: Rollout12.run(T), reset included, per cycle; *_off no velocity table, *_on the table, "
                   "*_on_horizon the table with the horizon-aware obstacle selection.  separation: one run each, the same "
                   "moving world; obs_vel_none re-reads the moved table every cycle and solves it as static."}
    print(json.dumps(res), flush=True)
    out = args.out if args.out is not None else os.path.join(ROOT, "profiles", "bench_rollout12_moving.json")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for w in worlds.values():
        w["solver"].close()


def sizes(args):
    """--sizes: see the module docstring."""
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs = 8, 20
    S = A // team
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    b = workload.make_batch12(A, N, "trot", seed=1234)
    sb = workload.make_scenes12(S, team, N, "trot", seed=1234, n_obs=scene_obs)
    goal = D(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    solves = (("no_table", False, False), ("obs_eps", True, False), ("obs_eps_clearance", True, True))
    worlds = {}
    for name, x0, g, phase, ob, scenes in (("one_team", b["x0"], goal, None, b["obstacles"], (0, 0)),
                                           ("scenes", sb["x0"], D(sb["goal"]), D(sb["phase"], torch.int32), sb["obstacles"],
                                            (team, scene_obs))):
        solver = srb12.Solver12(p, x0.shape[0], 0)
        solver.set_timing(False)
        solver.set_scenes(*scenes)
        ob = D(ob)
        eps, radius = (D(v) for v in workload.obstacle_sizes(ob.shape[0], 1234))
        mk = lambda e, c, r: srb12.Rollout12(solver, g, vref=workload.VREF, phase=phase, obstacles=ob,
                                             obs_eps=eps if e else None, obs_clearance=c, obs_radius=radius if r else None)
        worlds[name] = dict(solver=solver, x0=D(x0), ob=ob,
                            rolls={f"{k}{'_radius' if r else ''}": mk(e, c, r) for k, e, c in solves for r in (False, True)})

    def cycle(w, r):
        def f():
            r.reset(w["x0"])
            r.run(T)
        return f
    modes = [(f"{name}_{k}", cycle(w, r)) for name, w in worlds.items() for k, r in w["rolls"].items()]
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
            ms[name].append(1e3 * (time.perf_counter() - t0) / T)

    def stats(r):
        res = r.results()
        torch.cuda.synchronize(dev)
        d, fc, st = res["min_d_obs"].cpu().numpy(), res["fail_cycle"].cpu().numpy(), res["status"].cpu().numpy()
        ok = np.isin(st[..., 0], (0, 4)) & (st[..., 1] == 0)
        return {"clearance_to_bodies_m": {"smallest": float(d.min()), "median": float(np.median(d))},
                "agents_inside_a_body": {"at_cycle_0": int((fc == 0).sum()), "later": int((fc > 0).sum()),
                                         "never": int((fc < 0).sum())},
                "non_converged_solves": int((~ok).sum()), "solves": int(ok.size)}
    sep = {}
    for name, w in worlds.items():
        sep[name] = {}
        for k, _, _ in solves:
            cycle(w, w["rolls"][k + "_radius"])()
            sep[name][k] = stats(w["rolls"][k + "_radius"])
    spread = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res = {"tool": "tools/bench_rollout12.py --sizes", "agents": A, "horizon": N, "K_obs": Ko, "K_nbr": Kn,
           "scenes": {"n_scenes": S, "scene_agents": team, "scene_obs": scene_obs},
           "one_team_obstacles": int(worlds["one_team"]["ob"].shape[0]), "cycles_per_window": T, "rounds": args.rounds,
           "n_gpus": 1, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
           "separation_over_cycles": T, "separation": sep,
           "note": "ms_per_cycle: Rollout12.run(T), reset included, per cycle; *_no_table no level table, *_obs_eps the "
                   "drawn levels, *_obs_eps_clearance the levels with the clearance selection; *_radius: the metrics with "
                   "the body radii.  The three solves are three different NLPs: no target for these times.  separation: "
                   "one run each with obs_radius, the same world and the same bodies."}
    print(json.dumps(res), flush=True)
    out = args.out if args.out is not None else os.path.join(ROOT, "profiles", "bench_rollout12_sizes.json")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for w in worlds.values():
        w["solver"].close()


def agent_sizes(args):
    """--agents without a number: see the module docstring."""
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs = 8, 20
    S = A // team
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    b = workload.make_batch12(A, N, "trot", seed=1234)
    sb = workload.make_scenes12(S, team, N, "trot", seed=1234, n_obs=scene_obs)
    goal = D(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    solves = (("no_table", False, False), ("agent_rad_pad", True, False), ("agent_rad_pad_clearance", True, True))
    worlds = {}
    for name, x0, g, phase, ob, scenes in (("one_team", b["x0"], goal, None, b["obstacles"], (0, 0)),
                                           ("scenes", sb["x0"], D(sb["goal"]), D(sb["phase"], torch.int32), sb["obstacles"],
                                            (team, scene_obs))):
        solver = srb12.Solver12(p, x0.shape[0], 0)
        solver.set_timing(False)
        solver.set_scenes(*scenes)
        ob = D(ob)
        rad, pad, body = (D(v) for v in workload.agent_sizes(x0.shape[0], 1234))
        mk = lambda t, c, r: srb12.Rollout12(solver, g, vref=workload.VREF, phase=phase, obstacles=ob,
                                             agent_rad=rad if t else None, agent_pad=pad if t else None, nbr_clearance=c,
                                             agent_body=body if r else None)
        worlds[name] = dict(solver=solver, x0=D(x0), ob=ob,
                            rolls={f"{k}{'_body' if r else ''}": mk(t, c, r) for k, t, c in solves for r in (False, True)})

    def cycle(w, r):
        def f():
            r.reset(w["x0"])
            r.run(T)
        return f
    modes = [(f"{name}_{k}", cycle(w, r)) for name, w in worlds.items() for k, r in w["rolls"].items()]
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
            ms[name].append(1e3 * (time.perf_counter() - t0) / T)

    def stats(r):
        res = r.results()
        torch.cuda.synchronize(dev)
        d, cc, st = res["min_d_agent"].cpu().numpy(), res["collide_cycle"].cpu().numpy(), res["status"].cpu().numpy()
        ok = np.isin(st[..., 0], (0, 4)) & (st[..., 1] == 0)
        return {"clearance_between_bodies_m": {"smallest": float(d.min()), "median": float(np.median(d))},
                "agents_touching_a_body": {"at_cycle_0": int((cc == 0).sum()), "later": int((cc > 0).sum()),
                                           "never": int((cc < 0).sum())},
                "non_converged_solves": int((~ok).sum()), "solves": int(ok.size)}
    sep = {}
    for name, w in worlds.items():
        sep[name] = {}
        for k, _, _ in solves:
            cycle(w, w["rolls"][k + "_body"])()
            sep[name][k] = stats(w["rolls"][k + "_body"])
    spread = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res = {"tool": "tools/bench_rollout12.py --agents", "agents": A, "horizon": N, "K_obs": Ko, "K_nbr": Kn,
           "scenes": {"n_scenes": S, "scene_agents": team, "scene_obs": scene_obs},
           "one_team_obstacles": int(worlds["one_team"]["ob"].shape[0]), "cycles_per_window": T, "rounds": args.rounds,
           "n_gpus": 1, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
           "separation_over_cycles": T, "separation": sep,
           "note": "ms_per_cycle: Rollout12.run(T), reset included, per cycle; *_no_table no agent table, *_agent_rad_pad the "
                   "drawn radii and pads, *_agent_rad_pad_clearance those with the neighbour clearance selection; *_body: "
                   "the metrics with the body radii.  The three solves are three different NLPs: no target for these "
                   "times.  separation: one run each with agent_body, the same world and the same bodies."}
    print(json.dumps(res), flush=True)
    out = args.out if args.out is not None else os.path.join(ROOT, "profiles", "bench_rollout12_agents.json")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for w in worlds.values():
        w["solver"].close()


KICKS = (0.0, 0.02, 0.05, 0.1, 0.2)      # kick_v bounds (m/s per cycle): none, 7 %, 19 %, 37 %, 74 % of VREF
DYNTOL = 1e-8                            # SRB12_POL_DYNTOL: the dynamics residual of an accepted polish


def plant(args):
    """--plant: see the module docstring."""
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs, seed = 8, 20, 1234
    S = A // team
    A = S * team
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    sc = workload.replicate_scenes(workload.make_scenes12(1, team, N, "trot", seed=seed, n_obs=scene_obs), S)
    goal, phase, ob, x0 = D(sc["goal"]), D(sc["phase"], torch.int32), D(sc["obstacles"]), D(sc["x0"])
    solver = srb12.Solver12(p, A, 0)
    solver.set_timing(False)
    solver.set_scenes(team, scene_obs)
    P = srb12.Plant12

    def rollout(pl=None):
        return srb12.Rollout12(solver, goal, vref=workload.VREF, phase=phase, obstacles=ob, plant=pl)

    def run(r):
        r.reset(x0)
        r.run(T)

    def dist(v):
        v = np.asarray(v, dtype=float)
        return {"min": float(v.min()), "p05": float(np.quantile(v, 0.05)), "median": float(np.median(v)),
                "p95": float(np.quantile(v, 0.95)), "max": float(v.max())}

    def scene_stats(r):
        sr = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.scene_results().items()}
        z = r.results()["traj"][:, :, 2]
        return {"scenes_with_a_failure": int((sr["n_failed"] > 0).sum()), "n_failed": int(sr["n_failed"].sum()),
                "n_not_converged": int(sr["n_not_converged"].sum()), "solves": int(T * A),
                "min_d_obs": dist(sr["min_d_obs"]), "min_d_agent": dist(sr["min_d_agent"]),
                "height_m": {"min": float(z.min().item()), "max": float(z.max().item())}}

    # ---- safety: the sweep over kick_v bounds
    sweep = []
    for kick in KICKS:
        r = rollout(P(seed, kick_v=D(np.full(A, kick))))
        run(r)
        sweep.append(dict(kick_v=kick, **scene_stats(r)))

    # ---- linearisation: no kicks, the plant's equations at the model's point and at its own state
    lin = {}
    for name, at in (("at_state_0", False), ("at_state_1", True)):
        r = rollout(P(seed, mass=D(np.full(A, p.mass)), at_state=at))
        run(r)
        res = r.results()
        r2 = srb12.Rollout12(solver, goal, vref=workload.VREF, phase=phase, obstacles=ob, log_x=True,
                             plant=P(seed, mass=D(np.full(A, p.mass)), at_state=at))
        run(r2)
        res2 = r2.results()
        dep = (res2["traj"][1:] - res2["x"][:, :, 36:48]).abs()
        lin[name] = dict(scene_stats(r), largest_departure_from_the_prediction={
            "p_m": float(dep[:, :, 0:3].max().item()), "theta_rad": float(dep[:, :, 3:6].max().item()),
            "v_m_s": float(dep[:, :, 6:9].max().item()), "omega_rad_s": float(dep[:, :, 9:12].max().item()),
            "first_cycle_omega_rad_s": float(dep[0, :, 9:12].max().item())})
        del r2, res2, dep

    # ---- cost: interleaved
    kv, kp, kw, mass, inertia = (D(v) for v in workload.plant_tables12(A, seed))
    zero, mmodel = D(np.zeros(A)), D(np.full(A, p.mass))
    when, who = D(np.full(S, T // 2), torch.int32), D(team * np.arange(S), torch.int32)
    push = (when, who, D(np.tile([0.2, 0.1, 0.0, 0.0, 0.0, 0.3], (S, 1))))
    push0 = (when, who, D(np.zeros((S, 6))))
    modes = [("nominal", rollout()),
             ("plant_zero", rollout(P(seed, zero, zero, zero, pushes=push0))),
             ("plant_zero_mass", rollout(P(seed, zero, zero, zero, mass=mmodel, pushes=push0))),
             ("plant_zero_mass_at_state", rollout(P(seed, zero, zero, zero, mass=mmodel, at_state=True, pushes=push0))),
             ("plant", rollout(P(seed, kv, kp, kw, mass, inertia, pushes=push)))]
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
    out = {name: r.results() for name, r in modes}
    torch.cuda.synchronize(dev)
    iters = {name: float(o["iters"].double().sum(2).mean().item()) for name, o in out.items()}
    same = bool(torch.equal(out["nominal"]["traj"], out["plant_zero"]["traj"]))
    # a roll restarts every cycle from the logged state: per cycle it is within DYNTOL (1 + a + a^2 + a^3) of the
    # prediction where the solve was polished; the closed loop then carries the difference on, so the
    # trajectories are compared over the first cycle, where the two rollouts solved the same problems
    a = 1.0 + p.Ts * np.sqrt(2.0)
    tol = DYNTOL * (1 + a + a * a + a ** 3)
    ok0 = (out["nominal"]["status"][0, :, 1] == 0)
    d1 = (out["nominal"]["traj"][1] - out["plant_zero_mass"]["traj"][1]).abs().max(1).values
    roll_err = float(d1[ok0].max().item())
    roll_all = float((out["nominal"]["traj"] - out["plant_zero_mass"]["traj"]).abs().max().item())
    spread = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res = {"tool": "tools/bench_rollout12.py --plant", "agents": A, "horizon": N, "K_obs": Ko, "K_nbr": Kn,
           "batch": {"replicas": S, "team": team, "obstacles_per_scene": scene_obs}, "cycles": T, "rounds": args.rounds,
           "n_gpus": 1, "seed": seed, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
           "mean_iterations_per_solve": iters, "plant_zero_traj_equals_nominal": same,
           "plant_zero_mass_first_cycle_max_abs_diff_optimal": roll_err, "roll_tolerance": tol,
           "plant_zero_mass_traj_max_abs_diff_all_cycles": roll_all, "sweep": sweep, "linearisation": lin,
           "note": "ms_per_cycle: run(T) / T, reset included, interleaved: nominal (no plant: srb12_rollout_agents_device); "
                   "plant_zero (zero kick_v, kick_p, kick_w, one zero push per scene at cycle T / 2: the plant's two "
                   "kernels on nominal's states); plant_zero_mass (mass = the model's besides: the roll); "
                   "plant_zero_mass_at_state (the roll about the plant's own state: another plant, other NLPs); plant "
                   "(workload.plant_tables12 and one push per scene).  sweep: one rollout per kick_v bound (kick_v alone, "
                   "uniform over the agents), per-scene minima over the replicas.  linearisation: mass = the model's, no "
                   "kicks; the departure is max |next state - X at grid index 3| over the cycles and agents."}
    print(json.dumps(res), flush=True)
    out_path = args.out if args.out is not None else os.path.join(ROOT, "profiles", "bench_rollout12_plant.json")
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    solver.close()
    assert same, "the zero plant does not reproduce the nominal trajectory bit for bit"
    assert roll_err <= tol, f"the model's own roll leaves the prediction by {roll_err} (tolerance {tol})"


# (delay cycles, drop, noise_p m): tools/bench_link.py's settings, one factor at a time around the undegraded link
LINK_SETTINGS = ((0, 0.0, 0.0), (1, 0.0, 0.0), (2, 0.0, 0.0), (4, 0.0, 0.0), (0, 0.2, 0.0), (0, 0.5, 0.0), (0, 0.0, 0.03),
                 (0, 0.0, 0.1), (2, 0.2, 0.03))


def link(args):
    """--link: see the module docstring."""
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs, seed = 8, 20, 1234
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    spread = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    def dist(v):
        v = np.asarray(v, dtype=float)
        return {"min": float(v.min()), "p05": float(np.quantile(v, 0.05)), "median": float(np.median(v)),
                "p95": float(np.quantile(v, 0.95)), "max": float(v.max())}

    # ---- cost: the bench team, plans on
    b = workload.make_batch12(A, N, "trot", seed=seed)
    goal = D(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    x0, ob = D(b["x0"]), D(b["obstacles"])
    solver = srb12.Solver12(p, A, 0)
    solver.set_timing(False)
    delay, drop, noise_p, noise_v = workload.link_tables(A, seed)
    M = srbnmpc.LinkModel
    zero = lambda: M(seed=seed, delay=D(np.zeros(A, np.int32), torch.int32), drop=D(np.zeros(A)))
    full = lambda: M(seed=seed, delay=D(delay, torch.int32), drop=D(drop), noise_p=D(noise_p), noise_v=D(noise_v),
                     extrapolate=True)
    modes = [(name, srb12.Rollout12(solver, goal, vref=workload.VREF, obstacles=ob, plans=True, plan_selection=sel, link=ln))
             for name, sel, ln in (("nominal", False, None), ("link_zero", False, zero()), ("link", False, full()),
                                   ("nominal_selection", True, None), ("link_zero_selection", True, zero()),
                                   ("link_selection", True, full()))]

    def run(r, state=x0, cycles=T):
        r.reset(state)
        r.run(cycles)
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
    out = {name: r.results() for name, r in modes}
    torch.cuda.synchronize(dev)
    iters = {name: float(o["iters"].double().sum(2).mean().item()) for name, o in out.items()}
    same = bool(torch.equal(out["nominal"]["traj"], out["link_zero"]["traj"]))
    same_sel = bool(torch.equal(out["nominal_selection"]["traj"], out["link_zero_selection"]["traj"]))
    team_safety = {name: {"min_d_agent": float(o["min_d_agent"].min().item()), "min_d_obs": float(o["min_d_obs"].min().item())}
                   for name, o in out.items()}
    del modes, out
    solver.close()

    # ---- safety: replicas of one scene, one factor at a time, with and without the horizon-aware selection
    S = A // team
    A2 = S * team
    sc = workload.replicate_scenes(workload.make_scenes12(1, team, N, "trot", seed=seed, n_obs=scene_obs), S)
    goal2 = workload.cross_goals(sc["nbr_state"][:, :2], team, seed) if args.cross_goals else sc["goal"]
    goal2, phase2, ob2, x02 = D(goal2), D(sc["phase"], torch.int32), D(sc["obstacles"]), D(sc["x0"])
    body = D(np.full(A2, workload.FAIL_RADIUS * np.sqrt(workload.EPS_NBR) / (2 * np.sqrt(workload.EPS_OBS))))
    sweep = []
    for kn in args.safety_knbr:         # (K_nbr >= team - 1 selects every other agent of the scene, whatever the key)
        s2 = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=kn), A2, 0)
        s2.set_timing(False)
        s2.set_scenes(team, scene_obs)
        for d, q, e in LINK_SETTINGS:
            for ext in (False, True):
                if ext and d == 0 and q == 0.0:
                    continue                                  # nothing ages: extrapolate changes nothing
                for sel in (False, True):
                    ln = M(seed=seed, delay=D(np.full(A2, d, np.int32), torch.int32), drop=D(np.full(A2, q)),
                           noise_p=D(np.full(A2, e)), extrapolate=ext)
                    r2 = srb12.Rollout12(s2, goal2, vref=workload.VREF, phase=phase2, obstacles=ob2, plans=True,
                                         plan_selection=sel, agent_body=body, link=ln)
                    run(r2, x02, args.safety_cycles)
                    sr = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r2.scene_results().items()}
                    sweep.append({"K_nbr": kn, "delay": d, "drop": q, "noise_p": e, "extrapolate": int(ext),
                                  "plan_selection": int(sel), "agents_collided": int(sr["n_collided"].sum()),
                                  "agents_failed": int(sr["n_failed"].sum()),
                                  "solves_not_converged": int(sr["n_not_converged"].sum()),
                                  "scenes_with_a_collision": int((sr["n_collided"] > 0).sum()),
                                  "scenes_with_a_failure": int((sr["n_failed"] > 0).sum()),
                                  "max_age": int(r2.results()["link_age"].max().item()),
                                  "min_d_agent": dist(sr["min_d_agent"]), "min_d_obs": dist(sr["min_d_obs"])})
        s2.close()
    res = {"tool": "tools/bench_rollout12.py --link", "horizon": N, "K_obs": Ko, "K_nbr": Kn, "cycles": T,
           "rounds": args.rounds, "n_gpus": 1, "seed": seed,
           "cost": {"agents": A, "plans": True, "ms_per_cycle": {k: spread(v) for k, v in ms.items()},
                    "mean_iterations_per_solve": iters, "link_zero_traj_equals_nominal": same,
                    "link_zero_selection_traj_equals_nominal_selection": same_sel, "team": team_safety},
           "safety": {"replicas": S, "team": team, "obstacles_per_scene": scene_obs, "agents": A2,
                      "cycles": args.safety_cycles, "cross_goals": bool(args.cross_goals), "solves": int(A2 * args.safety_cycles),
                      "sweep": sweep},
           "note": "cost: run(T) / T, reset included, interleaved: nominal (no link: srb12_rollout_plant_device's path), "
                   "link_zero (delay and drop tables of zeros: srb12_rollout_link_device on nominal's states, the link's "
                   "launch and kernel alone), link (workload.link_tables with extrapolate: other NLPs from the second "
                   "cycle on); *_selection: the same three with plan_selection (under a link the selection's own plan is "
                   "the truth plan_table).  safety: one rollout of `safety.cycles` cycles per setting, every row at the "
                   "same delay / drop / noise_p, the distribution of the per-scene min_d_agent (clearance between bodies) "
                   "over the replicas, agents collided / failed and solves not converged summed over the replicas; "
                   "cross_goals: every agent's goal is the start of another agent of its scene."}
    print(json.dumps(res), flush=True)
    out_path = args.out if args.out is not None else os.path.join(ROOT, "profiles", "bench_rollout12_link.json")
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    assert same and same_sel, "a link of zero tables does not reproduce the nominal trajectory bit for bit"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=20, help="T: cycles per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1, help="untimed windows per mode")
    ap.add_argument("--agents", nargs="?", const="tables", default="1024",
                    help="with a number: the agent count (default 1024); without one: the agent-size measurement alone "
                         "(see above)")
    ap.add_argument("--agent-sizes", action="store_true", help="the agent-size measurement alone (as --agents without "
                                                               "a number; combines with --agents N)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--plans", action="store_true", help="add the plans-on modes (see above)")
    ap.add_argument("--outer", type=int, default=4, help="--plans: Jacobi rounds of the plan_change measurement")
    ap.add_argument("--moving", action="store_true", help="the moving-obstacle measurement alone (see above)")
    ap.add_argument("--vmax", type=float, default=1.0, help="--moving: the obstacles' top speed (m/s)")
    ap.add_argument("--sizes", action="store_true", help="the obstacle-size measurement alone (see above)")
    ap.add_argument("--plant", action="store_true", help="the disturbed-plant measurement alone (see above)")
    ap.add_argument("--link", action="store_true", help="the degraded-link measurement alone (see above)")
    ap.add_argument("--cross-goals", action="store_true", help="--link: goals exchanged within the scene")
    ap.add_argument("--safety-cycles", type=int, default=200, help="--link: cycles per rollout of the safety sweep")
    ap.add_argument("--safety-knbr", type=int, nargs="+", default=[8, 3],
                    help="--link: K_nbr of the safety sweep's solver, one sweep each (8 selects all 7 others of a scene of "
                         "8, so the two selections can differ in column order alone; 3 makes them choose)")
    args = ap.parse_args()
    if args.agents == "tables":
        args.agent_sizes, args.agents = True, "1024"
    args.agents = int(args.agents)
    if not torch.cuda.is_available():
        sys.exit("bench_rollout12.py needs a GPU (no CPU fallback)")
    if args.moving:
        return moving(args)
    if args.sizes:
        return sizes(args)
    if args.agent_sizes:
        return agent_sizes(args)
    if args.plant:
        return plant(args)
    if args.link:
        return link(args)
    dev = torch.device("cuda", 0)
    A, N, Ko, Kn, T = args.agents, 10, 3, 8, args.cycles
    team, scene_obs = 8, 20
    S = A // team
    D = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)

    b = workload.make_batch12(A, N, "trot", seed=1234)
    t = {k: D(v, torch.int32 if k == "contact" else torch.float64) for k, v in b.items()}
    goal = D(np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1)))
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    solver = srb12.Solver12(p, A, 0)
    solver.set_timing(False)
    roll = srb12.Rollout12(solver, goal, vref=workload.VREF, obstacles=t["obstacles"])
    plain_out = dict(x_qp=None, x=torch.zeros((A, p.nv), dtype=torch.float64, device=dev),
                     obj=torch.zeros(A, dtype=torch.float64, device=dev),
                     status=torch.zeros((A, 2), dtype=torch.int32, device=dev),
                     iters=torch.zeros((A, 2), dtype=torch.int32, device=dev))

    # the scene-batched team of the same size on a context of its own (the partition is a context setting)
    sb = workload.make_scenes12(S, team, N, "trot", seed=1234, n_obs=scene_obs)
    ssolver = srb12.Solver12(p, S * team, 0)
    ssolver.set_timing(False)
    ssolver.set_scenes(team, scene_obs)
    sroll = srb12.Rollout12(ssolver, D(sb["goal"]), vref=workload.VREF, phase=D(sb["phase"], torch.int32),
                            obstacles=D(sb["obstacles"]))
    sx0 = D(sb["x0"])

    # the LIP advance at the same agent count (the yardstick of the advance kernel: DESIGN.md 10.2)
    lb = workload.make_batch(A, N, 2, seed=1234)
    lsolver = srbnmpc.BatchSolver(srbnmpc.default_params(N, 2, K_obs=Ko, K_nbr=Kn), A, 0)
    lsolver.set_option("timing", 0)
    lroll = srbnmpc.Rollout(lsolver, goal, vref=workload.VREF, obstacles=t["obstacles"])
    lroll.reset(D(lb["x0"]))
    lroll.step()
    roll.reset(t["x0"])
    roll.step()
    lib, lib12 = srbnmpc.lib(), srb12._lib()

    def run():
        roll.reset(t["x0"])
        roll.run(T)

    def steps():
        roll.reset(t["x0"])
        for _ in range(T):
            roll.step()

    def plain():
        for _ in range(T):
            solver.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], plain_out)

    def scenes():
        sroll.reset(sx0)
        sroll.run(T)

    def advance12():                     # cycle 1 of the rollout left by the last rollout window: logs included
        sim, st = roll._sim(), solver._stream(None)
        for _ in range(T):
            lib12.srb12_sim_advance_device(solver._h, A, ctypes.byref(sim), 1, st)

    def metrics12():
        sim, st = roll._sim(), solver._stream(None)
        for _ in range(T):
            lib12.srb12_sim_metrics_device(solver._h, A, ctypes.byref(sim), 1, st)

    def advance_lip():
        sim, st = lroll._sim(), lsolver._stream(None)
        for _ in range(T):
            lib.srb_sim_advance_device(lsolver._h, A, ctypes.byref(sim), 1, st)

    modes = [("run", run), ("step", steps), ("plain_solve_loop", plain), ("scenes_run", scenes),
             ("advance12_kernel", advance12), ("metrics12_kernel", metrics12), ("advance_lip_kernel", advance_lip)]

    if args.plans:
        proll = srb12.Rollout12(solver, goal, vref=workload.VREF, obstacles=t["obstacles"], plans=True)
        hroll = srb12.Rollout12(solver, goal, vref=workload.VREF, obstacles=t["obstacles"], plans=True, plan_selection=True)
        sproll = srb12.Rollout12(ssolver, D(sb["goal"]), vref=workload.VREF, phase=D(sb["phase"], torch.int32),
                                 obstacles=D(sb["obstacles"]), plans=True)
        shroll = srb12.Rollout12(ssolver, D(sb["goal"]), vref=workload.VREF, phase=D(sb["phase"], torch.int32),
                                 obstacles=D(sb["obstacles"]), plans=True, plan_selection=True)

        def rolled(r, x0, stepwise=False):
            def f():
                r.reset(x0)
                if stepwise:
                    for _ in range(T):
                        r.step()
                else:
                    r.run(T)
            return f

        def shift12():
            for _ in range(T):
                solver.shift_plans_device(proll.out["plan"], proll.plan_table)
        modes += [("run_plans", rolled(proll, t["x0"])), ("step_plans", rolled(proll, t["x0"], True)),
                  ("run_plans_horizon_selection", rolled(hroll, t["x0"])), ("scenes_run_plans", rolled(sproll, sx0)),
                  ("scenes_run_plans_horizon_selection", rolled(shroll, sx0)), ("shift12_kernel", shift12)]
    for _ in range(args.warmup):
        for _, f in modes:
            f()
    torch.cuda.synchronize(dev)
    sec = {name: [] for name, _ in modes}
    for _ in range(args.rounds):
        for name, f in modes:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            sec[name].append(time.perf_counter() - t0)

    # untimed: the separation, the heights and the statuses over the rollout, one team and scene-batched
    run()
    r = roll.results()
    torch.cuda.synchronize(dev)
    safety = {"one_team": safety_of(r)}
    scenes()
    r = sroll.results()
    sc = sroll.scene_results()
    torch.cuda.synchronize(dev)
    safety["scenes"] = safety_of(r)
    safety["scenes"]["per_scene"] = {"min_d_agent": hist(sc["min_d_agent"].cpu().numpy()),
                                     "min_d_obs": hist(sc["min_d_obs"].cpu().numpy()),
                                     "scenes_with_a_failed_agent": int((sc["n_failed"] > 0).sum().item()),
                                     "scenes_with_a_non_converged_solve": int((sc["n_not_converged"] > 0).sum().item())}

    plans = None
    if args.plans:
        def per_scene(r):
            sc = r.scene_results()
            torch.cuda.synchronize(dev)
            return {"min_d_agent": hist(sc["min_d_agent"].cpu().numpy()), "min_d_obs": hist(sc["min_d_obs"].cpu().numpy()),
                    "scenes_with_a_failed_agent": int((sc["n_failed"] > 0).sum().item()),
                    "scenes_with_a_non_converged_solve": int((sc["n_not_converged"] > 0).sum().item())}
        for name, r, x0 in (("one_team_plans", proll, t["x0"]), ("one_team_plans_horizon_selection", hroll, t["x0"]),
                            ("scenes_plans", sproll, sx0), ("scenes_plans_horizon_selection", shroll, sx0)):
            r.reset(x0)
            r.run(T)
            res_ = r.results()
            torch.cuda.synchronize(dev)
            safety[name] = safety_of(res_)
            if name.startswith("scenes"):
                safety[name]["per_scene"] = per_scene(r)
        # plan_change per Jacobi round on the batch of the solve benchmark (fixed inputs, one cycle)
        cout = dict(plain_out, plan=torch.zeros((A, N, 2), dtype=torch.float64, device=dev))
        change = solver.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"],
                                             cout, outer=args.outer)
        torch.cuda.synchronize(dev)
        st = cout["status"].cpu().numpy()
        # the selection alone: the library's events around the selection launches of T solves, a context of its own
        tsolver = srb12.Solver12(p, A, 0)
        table = cout["plan"].clone()
        tout = dict(plain_out, x=torch.zeros_like(plain_out["x"]), plan=torch.zeros_like(table))
        sel_ms = {}
        for name, kw in (("snapshot", dict()), ("snapshot_with_table", dict(nbr_plan=table)),
                         ("horizon_aware", dict(nbr_plan=table, plan_selection=True))):
            v = []
            for i in range(T + 2):
                tsolver.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], tout, **kw)
                torch.cuda.synchronize(dev)
                if i >= 2:
                    v.append(tsolver.last_kernel_ms())
            v = np.array(v)
            sel_ms[name] = {"select_ms_median": float(np.median(v[:, 0])), "select_ms_min": float(v[:, 0].min()),
                            "select_ms_max": float(v[:, 0].max()), "solve_ms_median": float(np.median(v[:, 1]))}
        tsolver.close()
        plans = {"plan_change_per_jacobi_round_m": [float(c) for c in change.cpu().numpy()],
                 "jacobi_last_round_non_optimal_frac": float(1.0 - (np.isin(st[:, 0], (0, 4)) & (st[:, 1] == 0)).mean()),
                 "selection_alone_ms": sel_ms}

    cps = {k: {"median": float(np.median(T / np.array(v))), "min": float(np.min(T / np.array(v))),
               "max": float(np.max(T / np.array(v)))} for k, v in sec.items()}
    ms = {k: {"median": 1e3 / v["median"], "min": 1e3 / v["max"], "max": 1e3 / v["min"]} for k, v in cps.items()}
    res = {"tool": "tools/bench_rollout12.py", "agents": A, "horizon": N, "K_obs": Ko, "K_nbr": Kn,
           "scenes": {"n_scenes": S, "scene_agents": team, "scene_obs": scene_obs},
           "cycles_per_window": T, "rounds": args.rounds, "n_gpus": 1, "cycles_per_s": cps, "ms_per_cycle": ms,
           "overhead_ms_over_plain": {"run": ms["run"]["median"] - ms["plain_solve_loop"]["median"],
                                      "step": ms["step"]["median"] - ms["plain_solve_loop"]["median"]},
           "note": "run: Rollout12.run(T), the C driver; step: T x Rollout12.step(); plain_solve_loop: T x solve_device on "
                   "fixed inputs (no advance, metrics or carried state); scenes_run: Rollout12.run(T) of the scene-batched "
                   "team; *_kernel: T back-to-back calls of one entry point at cycle 1 (ms_per_cycle = ms per call).  A "
                   "rollout window includes its reset.",
           "safety": safety}
    if plans is not None:
        res["plans"] = plans
        res["plans"]["ms_per_cycle_over_plans_off"] = {
            k: ms[k]["median"] - ms[ref]["median"]
            for k, ref in (("run_plans", "run"), ("step_plans", "step"), ("run_plans_horizon_selection", "run"),
                           ("scenes_run_plans", "scenes_run"), ("scenes_run_plans_horizon_selection", "scenes_run"))}
        res["note"] += ("  *_plans: Rollout12(plans=True), the reference of each is the plans-off row of the same run; "
                        "shift12_kernel: T back-to-back srb12_shift_plans_device calls.")
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for s in (solver, ssolver, lsolver):
        s.close()


if __name__ == "__main__":
    main()
