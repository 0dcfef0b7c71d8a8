"""GPU tests of the disturbed plant (csrc/srb_plant.hip, srb_sim_advance_plant_device, srb_rollout_plant_device,
Rollout(kick_v=..., kick_p=..., plant_hcom=..., pushes=...)).

The kernel is compared bit for bit with its numpy restatement (tests/plant_oracle.py); the closed loop is checked
per cycle from the device's own logs, so nothing drifts: the next state is the restatement applied to the logged state
and solution, bitwise, and every solve agrees with the plan oracle on the logged state as in test_rollout_gpu.py."""
import ctypes

import numpy as np
import pytest

import plan_oracle
import plant_oracle
import sim_oracle
import srbnmpc
import test_plant
import test_rollout_gpu as trg
from srbnmpc import workload

gpu = pytest.mark.gpu
TS = workload.TS
NLP_TOL = trg.NLP_TOL
EQTOL = 1e-8          # SRB_POLISH_EQTOL (csrc/srb_kernel_params.h): lip_eq_res, the largest ABSOLUTE equality residual
_need_gpu, solver, dev, host, xus = trg._need_gpu, trg.solver, trg.dev, trg.host, trg.xus


def _dp(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._dp)


def _ip(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._ip)


# ================================================================================== 1. the kernel, bitwise
@gpu
@pytest.mark.parametrize("A,N,C,what,with_phase,offset,n_all",
                         [(5, 4, 2, "kick_v", False, 0, 5), (300, 10, 2, "all", True, 7, 320),
                          (300, 4, 4, "hcom", False, 0, 300)])
def test_kernel_equals_the_restatement_bitwise(A, N, C, what, with_phase, offset, n_all):
    """srb_sim_advance_plant_device at a first cycle (the caller's state, nothing of the plant) and at a later one,
    random x as the previous solution: every output array against numpy.  A = 300 is a partial second block; the
    shard of case two starts at global row 7 of 320; its six pushes hold two on one agent in the firing cycle (they
    add up in table order), one on a row outside the shard, one in another cycle, one at c_first and one single."""
    torch = _need_gpu()
    s = solver(N, C, 1, 0)
    p, nv = s.params, s.params.nv
    rng = np.random.default_rng(1000 + A + N + C)
    state = np.stack([rng.uniform(0, 9, A), rng.uniform(-.3, .3, A), rng.uniform(-2, 2, A), rng.uniform(-.3, .3, A)], 1)
    goal = np.tile([10.0, 0.0], (A, 1))
    phase = rng.integers(0, 4, A).astype(np.int32) if with_phase else None
    x = rng.normal(size=(A, nv)); x[:, 12] = rng.uniform(0, 9, A); x[:, 14] = rng.uniform(-2, 2, A)
    x[:, 4 * N:6 * N] = rng.uniform(-0.3, 0.3, (A, 2 * N))
    status = rng.integers(0, 5, (A, 2)).astype(np.int32); iters = rng.integers(0, 50, (A, 2)).astype(np.int32)
    c0, c1, seed = 3, 6, 0x1234567890abcdef
    kick_v = rng.uniform(0.0, 0.1, n_all) if what in ("kick_v", "all") else None
    kick_p = rng.uniform(0.0, 0.02, n_all) if what == "all" else None
    hcom = p.hcom * rng.uniform(0.8, 1.2, n_all) if what in ("hcom", "all") else None
    pushes = None
    if what == "all":
        pushes = (np.array([c1, c1, c1, c1 + 1, c0, c1], np.int32), np.array([offset + 4, 3, offset + 4, offset + 9, offset + 5, offset + 299], np.int32),
                  rng.uniform(-0.3, 0.3, (6, 2)))
    f8, i4 = torch.float64, torch.int32
    z = lambda *sh, dt=f8: torch.full(sh, -7, dtype=dt, device="cuda")
    t = dict(state=dev(torch, state), goal=dev(torch, goal), phase=None if phase is None else dev(torch, phase),
             x=dev(torch, x), status=dev(torch, status), iters=dev(torch, iters), x0=z(A, 4), ref=z(A, 4 * N),
             foot=z(A, N, 2, C), last_state=z(A, 4), alpha_buf=z(A, 4), plan_table=z(A, N, 2), traj=z(c1 - c0 + 1, A, 4),
             status_log=z(c1 - c0, A, 2, dt=i4), iters_log=z(c1 - c0, A, 2, dt=i4), x_log=z(c1 - c0, A, nv),
             nbr=z(n_all, 4), dist_log=z(c1 - c0, A, 4),
             kick_v=None if kick_v is None else dev(torch, kick_v), kick_p=None if kick_p is None else dev(torch, kick_p),
             hcom=None if hcom is None else dev(torch, hcom))
    pt = [None] * 3 if pushes is None else [dev(torch, v) for v in pushes]
    sim = srbnmpc.Sim(_dp(t["state"]), _dp(t["goal"]), _ip(t["phase"]), 0.27, c0, _dp(t["x"]), _ip(t["status"]),
                      _ip(t["iters"]), _dp(t["x0"]), _dp(t["ref"]), _dp(t["foot"]), _dp(t["last_state"]),
                      _dp(t["alpha_buf"]), _dp(t["plan_table"]), _dp(t["traj"]), _ip(t["status_log"]),
                      _ip(t["iters_log"]), _dp(t["x_log"]), None, _dp(t["nbr"]), 0, n_all, offset, None, None, None, None,
                      None, None)
    plant = srbnmpc.Plant(seed, _dp(t["kick_v"]), _dp(t["kick_p"]), _dp(t["hcom"]), 0 if pushes is None else 6,
                          _ip(pt[0]), _ip(pt[1]), _dp(pt[2]), _dp(t["dist_log"]))
    lib, st = srbnmpc.lib(), s._stream(None)
    for c in (c0, c1):
        srbnmpc._check(lib.srb_sim_advance_plant_device(s._h, A, ctypes.byref(sim), ctypes.byref(plant), c, st))
        torch.cuda.synchronize()
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}
        if c == c0:
            w = sim_oracle.advance(N, C, TS, state, goal, 0.27, c, phase)
            w["state"] = state
            assert (got["plan_table"] == -7).all() and (got["x_log"] == -7).all() and (got["dist_log"] == -7).all()
        else:
            w = plant_oracle.advance_plant(N, C, TS, p.grav, 0.27, c, state, x, goal, phase, agent_offset=offset,
                                           seed=seed, kick_v=kick_v, kick_p=kick_p, plant_hcom=hcom, pushes=pushes)
            r = c - c0 - 1
            np.testing.assert_array_equal(got["dist_log"][r], w["dist"])
            assert (got["dist_log"][:r] == -7).all() and (got["traj"][1:c - c0] == -7).all()
            np.testing.assert_array_equal(got["plan_table"], w["plan_table"])
            np.testing.assert_array_equal(got["status_log"][r], status)
            np.testing.assert_array_equal(got["iters_log"][r], iters)
            np.testing.assert_array_equal(got["x_log"][r], x)
        for k in ("state", "x0", "ref", "foot", "last_state"):
            np.testing.assert_array_equal(got[k], w[k], err_msg=f"cycle {c}: {k}")
        np.testing.assert_array_equal(got["alpha_buf"], w["state"])
        np.testing.assert_array_equal(got["traj"][c - c0], w["state"])
    d = w["dist"]
    if what == "kick_v":
        assert (d[:, [0, 2]] == 0).all() and (d[:, [1, 3]] != 0).all() and (np.abs(d[:, 1]) < kick_v).all()
        np.testing.assert_array_equal(w["state"][:, [0, 2]], x[:, [12, 14]])
    if what == "hcom":
        assert (d == 0).all() and (w["state"] != x[:, 12:16]).all()           # the roll, not the prediction
    if what == "all":
        u = plant_oracle.kicks(seed, c1, offset + np.arange(A))
        both = (0.0 + kick_v[offset + 4] * u[4, 0] + pushes[2][0, 0]) + pushes[2][2, 0]     # table order
        assert d[4, 1] == both and d[299, 1] == 0.0 + kick_v[offset + 299] * u[299, 0] + pushes[2][5, 0]
        assert d[9, 1] == 0.0 + kick_v[offset + 9] * u[9, 0] and d[5, 1] == 0.0 + kick_v[offset + 5] * u[5, 0]


# ================================================================================== the closed loop
def drive(r, T, plant=None, agents_entry=False):
    """T cycles of the Rollout r (after reset) by the C driver, called directly: srb_rollout_agents_device, or
    srb_rollout_plant_device with `plant` (None, or a srbnmpc.Plant)."""
    s, o = r.solver, r.out
    r._reserve(T)
    b = srbnmpc.Batch(None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], r.A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, _dp(o["alpha"]), None, 0, None,
                      _dp(o.get("plan")))
    lib = srbnmpc.lib()
    if agents_entry:
        rc = lib.srb_rollout_agents_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), None, None, None, T,
                                           s._stream(None))
    else:
        rc = lib.srb_rollout_plant_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), None, None, None,
                                          None if plant is None else ctypes.byref(plant), T, s._stream(None))
    srbnmpc._check(rc)
    r.c, r.flushed = T, True
    return host(r.results())


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_nothing_set_is_the_old_path_bitwise(plans):
    """plant NULL, and a struct of NULL tables with n_push 0 (and a dist_log, which then stays unwritten), give the bits
    of srb_rollout_agents_device: traj, the logs and every metric, 16 agents, 6 cycles."""
    torch = _need_gpu()
    A, N, C, Ko, Kn, _, seed, _ = sim_oracle.RUNS[0]
    T = 6
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    dist = torch.full((T, A, 4), -7.0, dtype=torch.float64, device="cuda")
    empty = srbnmpc.Plant(99, None, None, None, 0, None, None, None, _dp(dist))
    res = []
    for kw in (dict(agents_entry=True), dict(plant=None), dict(plant=empty)):
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles))
        r.reset(dev(torch, state))
        res.append(drive(r, T, **kw))
    assert "disturbance" not in res[0] and (dist == -7).all()
    for other in res[1:]:
        assert sorted(other) == sorted(res[0])
        for k, v in res[0].items():
            assert np.array_equal(other[k], v), k
    assert res[0]["traj"].shape == (T + 1, A, 4) and not np.array_equal(res[0]["traj"][T], res[0]["traj"][0])


def plant_setup(torch, run, what="all", seed=11):
    """The disturbed team of one of sim_oracle.RUNS: kick_v 0.05, kick_p 0.01, the mismatched heights of
    workload.plant_tables and one push; host tables and the Rollout keyword arguments."""
    A, N, C, Ko, Kn, T, team_seed, plans = run
    state, goal, obstacles = sim_oracle.team(A, N, C, team_seed)
    tab = dict(kick_v=np.full(A, 0.05), kick_p=np.full(A, 0.01), plant_hcom=workload.plant_tables(A, 3)[2],
               pushes=(np.array([3], np.int32), np.array([5], np.int32), np.array([[0.15, -0.1]])))
    kw = dict(plant_seed=seed, kick_v=dev(torch, tab["kick_v"]), kick_p=dev(torch, tab["kick_p"]),
              plant_hcom=dev(torch, tab["plant_hcom"]), pushes=tuple(dev(torch, v) for v in tab["pushes"]))
    return state, goal, obstacles, tab, kw


_rolls = {}


def disturbed(run, mode="run"):
    """The disturbed rollout of `run` on the device with log_x, once per (run, mode): host copies of results()."""
    if (run, mode) not in _rolls:
        torch = _need_gpu()
        A, N, C, Ko, Kn, T, _, plans = run
        state, goal, obstacles, tab, kw = plant_setup(torch, run)
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles),
                            **kw)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        _rolls[(run, mode)] = host(r.results())
    return _rolls[(run, mode)]


@gpu
def test_the_model_is_its_own_plant():
    """plant_hcom = params.hcom everywhere, no kicks, no pushes: wherever the NLP stage is OPTIMAL (polished: its
    equality rows X_k = Ad X_{k-1} + Bd U_k hold to EQTOL, absolute), the plant's roll from x0 under U_0 .. U_3 ends at
    X_3 to within the residuals propagated through three further steps, EQTOL (1 + |Ad| + |Ad|^2 + |Ad|^3), |.| the
    infinity norm of the plant's own Ad.  A wrong choice of U entries misses this by centimetres."""
    torch = _need_gpu()
    A, N, C, Ko, Kn, _, seed, _ = sim_oracle.RUNS[0]
    T = 6
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    s = solver(N, C, Ko, Kn)
    r = srbnmpc.Rollout(s, dev(torch, goal), log_x=True, obstacles=dev(torch, obstacles),
                        plant_hcom=dev(torch, np.full(A, s.params.hcom)))
    r.reset(dev(torch, state))
    r.run(T)
    res = host(r.results())
    Ad, _ = plant_oracle.lip(s.params.grav, np.array([s.params.hcom]), s.params.Ts)
    na = np.abs(Ad[0]).sum(1).max()
    bound = EQTOL * (1 + na + na ** 2 + na ** 3)
    err = np.abs(res["traj"][1:] - res["x"][:, :, 12:16]).max(2)             # [T][A]
    opt = res["status"][:, :, 1] == 0
    print(f"|Ad|inf {na:.6f} bound {bound:.3e}; OPTIMAL {opt.sum()} of {opt.size}: max |roll - X3| {err[opt].max():.3e}"
          f" (all cycles {err.max():.3e})")
    assert opt.sum() >= opt.size // 2 and (res["disturbance"] == 0).all()
    assert err[opt].max() <= bound, (err[opt].max(), bound)
    assert (res["traj"][1:] != res["x"][:, :, 12:16]).any()                  # ... and it is the roll that was stored


@gpu
def test_disturbed_closed_loop_every_cycle_from_the_logs():
    run = sim_oracle.RUNS[1]
    A, N, C, Ko, Kn, T, _, plans = run
    torch = _need_gpu()
    state, goal, obstacles, tab, _ = plant_setup(torch, run)
    res = disturbed(run)
    p = sim_oracle.closed_loop(run)["p"]
    assert res["cycles"] == T and res["disturbance"].shape == (T, A, 4) and np.array_equal(res["traj"][0], state)
    worst = 0.0
    for c in range(T):
        b, table = sim_oracle.cycle_inputs(p, res["traj"][c], goal, obstacles, c, res["x"][c - 1] if c else None, plans)
        o = plan_oracle.solve(p, b, table)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        worst = max(worst, np.abs(xus(N, res["x"][c]) - xus(N, o["x"])).max())
        np.testing.assert_allclose(xus(N, res["x"][c]), xus(N, o["x"]), atol=NLP_TOL, rtol=0, err_msg=f"cycle {c}")
        st, d = plant_oracle.plant_state(N, TS, p.grav, c + 1, res["traj"][c], res["x"][c], seed=11, **tab)
        np.testing.assert_array_equal(res["traj"][c + 1], st, err_msg=f"cycle {c}")
        np.testing.assert_array_equal(res["disturbance"][c], d, err_msg=f"cycle {c}")
    assert np.array_equal(res["state"], res["traj"][T])
    d = res["disturbance"]
    assert d[2, 5, 1] != 0 and np.abs(d[:, :, [1, 3]]).max() <= 0.05 + 0.15 and np.abs(d[:, :, [0, 2]]).max() < 0.01
    off = np.abs(res["traj"][1:] - res["x"][:, :, 12:16]).max()
    print(f"run {run}: max |X,U,s - oracle| over {T} disturbed cycles = {worst:.3e}; largest departure from the "
          f"prediction {off:.4f}; min_d_agent {res['min_d_agent'].min():.4f} min_d_obs {res['min_d_obs'].min():.4f}")
    assert off > 0.01


@gpu
def test_c_driver_equals_python_steps_bitwise_with_the_plant_and_plans():
    a, b = disturbed(sim_oracle.RUNS[1], "run"), disturbed(sim_oracle.RUNS[1], "step")
    assert sorted(a) == sorted(b) and "disturbance" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@gpu
def test_shards_reproduce_the_full_team_bitwise_with_every_plant_table():
    """As test_rollout_gpu.test_shards_reproduce_the_full_team_bitwise: two shards (cut at 7) with the whole plant
    tables each, the all-gather stood in for by torch.cat, against the full team's run(); the push is on row 9, so it
    fires in the second shard at its local row 2."""
    torch = _need_gpu()
    run = sim_oracle.RUNS[0]
    A, N, C, Ko, Kn, _, _, _ = run
    state, goal, obstacles, tab, kw = plant_setup(torch, run)
    kw["pushes"] = (dev(torch, np.array([2], np.int32)), dev(torch, np.array([9], np.int32)), dev(torch, np.array([[0.2, 0.1]])))
    ob = dev(torch, obstacles)
    full = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), log_x=True, obstacles=ob, **kw)
    full.reset(dev(torch, state))
    full.run(3)
    want = host(full.results())
    assert want["disturbance"][1, 9, 1] != 0 and (want["disturbance"][:, :, 1] != 0).all()
    cut, sh = 7, []
    for lo, hi in ((0, cut), (cut, A)):
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), hi - lo)
        r = srbnmpc.Rollout(s, dev(torch, goal[lo:hi]), log_x=True, obstacles=ob, agent_offset=lo, n_all=A, **kw)
        r.reset(dev(torch, state[lo:hi]))
        sh.append(r)
    for _ in range(3):
        for r in sh:
            r.advance()
        table = torch.cat([r.last_state for r in sh]).contiguous()
        for r in sh:
            r.step(exchange=lambda local, table=table: table)
    got = [host(r.results()) for r in sh]
    for k, v in want.items():
        if k == "cycles":
            assert got[0][k] == got[1][k] == 3
            continue
        cat = np.concatenate([g[k] for g in got], 1 if v.ndim > 1 and k not in ("state",) else 0)
        assert np.array_equal(cat, v), k
    for r in sh:
        r.solver.close()


@gpu
def test_replicas_of_one_scene_draw_by_their_global_rows():
    """workload.replicate_scenes of one 4-agent scene x 8 under set_scenes: without kicks every replica is the same
    rollout; with kick_v 0.05 every replica has its own draws, the restatement's at its global rows; the same seed
    gives the same bits, another seed another disturbance."""
    torch = _need_gpu()
    team, n_obs, copies, N, C, T = 4, 5, 8, 4, 2, 4
    sc = workload.replicate_scenes(workload.make_scenes(1, team, N, C, seed=2, n_obs=n_obs), copies)
    A = team * copies
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=1, K_nbr=2), A)
    s.set_scenes(team, n_obs)

    def roll(kick, seed):
        r = srbnmpc.Rollout(s, dev(torch, sc["goal"]), phase=dev(torch, sc["phase"]), log_x=True,
                            obstacles=dev(torch, sc["obstacles"]), kick_v=dev(torch, np.full(A, kick)), plant_seed=seed)
        r.reset(dev(torch, sc["x0"]))
        r.run(T)
        out = host(r.results())
        out["scenes"] = host(r.scene_results())
        return out
    calm = roll(0.0, 5)
    per = calm["traj"].reshape(T + 1, copies, team, 4)
    assert (calm["disturbance"] == 0).all() and (per == per[:, :1]).all()
    a, again, other = roll(0.05, 5), roll(0.05, 5), roll(0.05, 6)
    for k in a:
        if k != "scenes":
            assert np.array_equal(a[k], again[k]), k
    assert not np.array_equal(a["disturbance"], other["disturbance"])
    d = a["disturbance"].reshape(T, copies, team, 4)
    for i in range(copies):
        for j in range(i):
            assert (d[:, i] != d[:, j])[..., [1, 3]].all(), (i, j)
    p = s.params
    for c in range(T):
        st, dd = plant_oracle.plant_state(N, TS, p.grav, c + 1, a["traj"][c], a["x"][c], seed=5, kick_v=np.full(A, 0.05))
        np.testing.assert_array_equal(a["disturbance"][c], dd)
        np.testing.assert_array_equal(a["traj"][c + 1], st)
    assert a["scenes"]["n_scenes"] == copies and a["scenes"]["min_d_agent"].shape == (copies,)
    s.close()


@gpu
def test_refusals_by_name_on_a_live_context_and_it_survives():
    torch = _need_gpu()
    run = sim_oracle.RUNS[2]
    A, N, C, Ko, Kn, T, seed, plans = run
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    s = solver(N, C, Ko, Kn)
    r = srbnmpc.Rollout(s, dev(torch, goal), plans=True, log_x=True, obstacles=dev(torch, obstacles))
    r.reset(dev(torch, state))
    r._reserve(2)
    lib = srbnmpc.lib()
    err = lambda: lib.srb_last_error().decode()
    o = r.out
    b = srbnmpc.Batch(None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, _dp(o["x"]), _dp(o["obj"]),
                      _ip(o["status"]), _ip(o["iters"]), None, _dp(o["alpha"]), None, 0, None, _dp(o["plan"]))
    keep, cases = test_plant.refusal_cases()
    for plant, word, sim_x in cases:
        sim = r._sim()
        if sim_x:
            sim.x = None
        else:
            assert test_plant.call_refused(lib, s._h, "rollout", plant, sim, b, A) == -1 and word in err(), word
        assert test_plant.call_refused(lib, s._h, "advance", plant, sim, None, A) == -1 and word in err(), word
    tab = dev(torch, np.full(A + 1, 0.01))
    on = srbnmpc.Plant(1, _dp(tab), None, None, 0, None, None, None, None)
    sim = r._sim(); sim.agent_offset = 2                       # rows 2 .. A + 1 of an A-row table
    assert lib.srb_sim_advance_plant_device(s._h, A, ctypes.byref(sim), ctypes.byref(on), 1, s._stream(None)) == -1
    assert "srb_plant: agent_offset + n_agents exceeds n_all" in err()
    b.agent_offset = 1                                         # a shard cannot roll out alone, plant or not
    assert test_plant.call_refused(lib, s._h, "rollout", on, r._sim(), b, A) == -1 and "sharded" in err()
    for name, bad, word in (("kick_v", dev(torch, np.full(A, -0.1)), "kick_v must be >= 0"),
                            ("kick_p", dev(torch, np.full(A + 1, 0.1)), "kick_p"),
                            ("plant_hcom", dev(torch, np.zeros(A)), "plant_hcom must be > 0"),
                            ("plant_hcom", dev(torch, np.full(A, np.nan)), "plant_hcom must be finite"),
                            ("kick_v", np.full(A, 0.1), "kick_v"),
                            ("pushes", (dev(torch, np.array([1], np.int32)), dev(torch, np.array([A], np.int32)),
                                        dev(torch, np.zeros((1, 2)))), "pushes: agent"),
                            ("pushes", (dev(torch, np.array([1], np.int32)),) * 2, "pushes must be a triple"),
                            ("plant_seed", -1, "plant_seed")):
        with pytest.raises(ValueError, match=word):
            srbnmpc.Rollout(s, dev(torch, goal), obstacles=dev(torch, obstacles), **{name: bad})
    # after the refusals a plain rollout on the same context gives the bits it always gave
    r.reset(dev(torch, state))
    r.run(T)
    res = host(r.results())
    want = trg.rollout(run)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
