"""GPU tests of the degraded neighbour link (csrc/srb_link.hip, srb_link_update_device, srb_rollout_link_device,
Rollout(link=srbnmpc.LinkModel(...))).

The kernel is compared bit for bit with its numpy restatement (tests/link_oracle.py), state buffers included; the closed
loop is checked per cycle from the device's own logs: what is seen is the restatement applied to the logged truth,
bitwise, every solve agrees with the plan oracle fed the PERCEIVED tables to test_rollout_gpu.py's tolerance, and the
metrics are sim_oracle's on the TRUE states."""
import ctypes

import numpy as np
import pytest

import link_oracle
import plan_oracle
import sim_oracle
import srbnmpc
import test_rollout_gpu as trg
from srbnmpc import workload

gpu = pytest.mark.gpu
TS = workload.TS
NLP_TOL = trg.NLP_TOL
_need_gpu, solver, dev, host, xus = trg._need_gpu, trg.solver, trg.dev, trg.host, trg.xus
FILL, GUARD = -7, 64


def _dp(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._dp)


def _ip(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._ip)


def guarded(torch, shape, dtype):
    """A sentinel-filled buffer of `shape` at the front of an allocation with GUARD more elements behind it."""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), FILL, dtype=dtype, device="cuda")
    return flat, flat[:n].view(*shape)


def link_buffers(torch, n, N, D, T):
    f8, i4 = torch.float64, torch.int32
    shapes = dict(ring_state=((D + 1, n, 4), f8), ring_plan=((D + 1, n, N, 2), f8), held_state=((n, 4), f8),
                  held_plan=((n, N, 2), f8), held_cycle=((n,), i4), seen_state=((n, 4), f8), seen_plan=((n, N, 2), f8),
                  age_log=((T, n), i4))
    flat, view = {}, {}
    for k, (sh, dt) in shapes.items():
        flat[k], view[k] = guarded(torch, sh, dt)
    return flat, view


def link_struct(torch, tab, buf, dtab):
    """srbnmpc.Link of the host tables `tab` (link_oracle.tables) on the device buffers `buf`; dtab keeps the device
    copies of the tables alive."""
    for k in ("delay", "drop", "noise_p", "noise_v"):
        dtab[k] = None if tab[k] is None else dev(torch, tab[k])
    return srbnmpc.Link(tab["seed"], _ip(dtab["delay"]), _dp(dtab["drop"]), _dp(dtab["noise_p"]), _dp(dtab["noise_v"]),
                        tab["max_delay"], tab["extrapolate"], _dp(buf["ring_state"]), _dp(buf["ring_plan"]),
                        _dp(buf["held_state"]), _dp(buf["held_plan"]), _ip(buf["held_cycle"]), _dp(buf["seen_state"]),
                        _dp(buf["seen_plan"]), _ip(buf["age_log"]))


# ================================================================================== 1. the kernel, bitwise
def kernel_case(name, rng):
    """(n, N, c_first, cycles, plans, tables) of the three cases."""
    seed = 0xfedcba9876543210
    if name == "noise":
        n, N = 5, 4
        return n, N, 3, 4, True, link_oracle.tables(seed, None, None, rng.uniform(0, 0.03, n), rng.uniform(0, 0.05, n), 0, 0)
    if name == "all":
        n, N, D = 300, 10, 3
        delay = rng.integers(0, D + 1, n).astype(np.int32)
        delay[:6] = [0, D, D + 5, -2, 1, 2]                    # two entries outside the ring: clamped
        drop = rng.uniform(0, 0.5, n)
        drop[:7], drop[7] = 0.0, 1.0
        return n, N, 3, 10, True, link_oracle.tables(seed, delay, drop, rng.uniform(0, 0.03, n), rng.uniform(0, 0.05, n), D, 1)
    n, N = 300, 4
    drop = rng.uniform(0, 1, n)
    drop[:4] = [0.0, 1.0, 0.0, 1.0]
    return n, N, 3, 6, False, link_oracle.tables(seed, None, drop, None, None, 0, 1)


@gpu
@pytest.mark.parametrize("name", ["noise", "all", "drop"])
def test_kernel_equals_the_restatement_bitwise(name):
    """srb_link_update_device over consecutive cycles with random truth tables per cycle, no solve: seen tables, age and
    every state buffer against numpy after every cycle, for the product mapping and for every stated one (1, 8, 16
    threads per row).  n_all = 300 is a partial second block; with max_delay 3 the ring wraps at least twice over cycles
    3 .. 12; "drop" has no plan table.  Every buffer starts at a sentinel with a guard behind it: what the restatement
    leaves alone stays the sentinel, and so does the guard."""
    torch = _need_gpu()
    rng = np.random.default_rng(2000 + len(name))
    n, N, c0, T, plans, tab = kernel_case(name, rng)
    s = solver(N, 2, 1, 0)
    st = np.stack([rng.uniform(0, 9, (T, n)), rng.uniform(-2, 2, (T, n)), rng.uniform(-.3, .3, (T, n)),
                   rng.uniform(-.3, .3, (T, n))], -1)
    pl = rng.uniform(-3, 12, (T, n, N, 2))
    want = link_oracle.run(c0, st, pl if plans else None, tab, N, FILL)
    lib, stream = srbnmpc.lib(), s._stream(None)
    d_st, d_pl = dev(torch, st), dev(torch, pl)
    for lanes in (0, 1, 8, 16):                               # 0: srb_link_update_device itself
        flat, buf = link_buffers(torch, n, N, tab["max_delay"], T + 1)
        keep = {}
        link = link_struct(torch, tab, buf, keep)
        for i in range(T):
            args = (s._h, n, ctypes.byref(link), _dp(d_st[i]), _dp(d_pl[i]) if plans else None, c0 + i, c0)
            srbnmpc._check(lib.srb_link_update_lanes_device(*args, lanes, stream) if lanes else
                           lib.srb_link_update_device(*args, stream))
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in buf.items()}
            seen, seen_plan, age, state = want[i]
            msg = f"{name}: lanes {lanes}, cycle {c0 + i}"
            np.testing.assert_array_equal(got["seen_state"], seen, err_msg=msg)
            np.testing.assert_array_equal(got["age_log"][i], age, err_msg=msg)
            assert (got["age_log"][i + 1:] == FILL).all(), msg
            if seen_plan is None:
                prev = want[i - 1][1] if i and plans else None
                assert (got["seen_plan"] == FILL).all() if prev is None else np.array_equal(got["seen_plan"], prev), msg
            else:
                np.testing.assert_array_equal(got["seen_plan"], seen_plan, err_msg=msg)
            for k, v in state.items():
                np.testing.assert_array_equal(got[k], v, err_msg=f"{msg}: {k}")
        for k, v in flat.items():
            assert (v[-GUARD:] == FILL).all(), (name, lanes, k)
    ages = np.array([w[2] for w in want])
    if name == "noise":
        assert (ages == 0).all() and all((w[0] != st[i]).all() for i, w in enumerate(want))
        assert all(np.abs(w[0] - st[i])[:, :2].max() < 0.03 for i, w in enumerate(want))
    if name == "all":
        assert ages.max() > 3 and (ages[:, 7] == np.arange(T)).all() and (ages[:, 6] == np.minimum(tab["delay"][6], np.arange(T))).all()
        assert (ages[4:, 2] == 3).all() and (ages[:, 3] == 0).all()                    # clamped into 0 .. max_delay
    if name == "drop":
        assert (ages[:, [0, 2]] == 0).all() and (ages[:, [1, 3]] == np.arange(T)[:, None]).all()
        assert (want[-1][3]["ring_plan"] == FILL).all() and (want[-1][3]["held_plan"] == FILL).all()


# ================================================================================== the closed loop
def team_kw(torch, run):
    A, N, C, Ko, Kn, T, seed, plans = run
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    return state, goal, obstacles


def roll(torch, run, T, link=None, mode="run", **kw):
    A, N, C, Ko, Kn, _, _, plans = run
    state, goal, obstacles = team_kw(torch, run)
    r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles),
                        link=link, **kw)
    r.reset(dev(torch, state))
    if mode == "run":
        r.run(T)
    else:
        for _ in range(T):
            r.step()
    out = host(r.results())
    if r.seen_state is not None:
        out["seen_state"] = r.seen_state.cpu().numpy()
        out["last_state"] = r.last_state.cpu().numpy()
    if r.seen_plan is not None:
        out["seen_plan"] = r.seen_plan.cpu().numpy()
    return out


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_a_link_that_degrades_nothing_is_the_plain_rollout_bitwise(plans):
    """delay zeros and drop zeros, no noise, extrapolate 0 and 1: the kernel runs (seen_state is written: it is the last
    cycle's truth) and the rollout has the bits of the plain one, 16 agents, 6 cycles."""
    torch = _need_gpu()
    run = sim_oracle.RUNS[1 if plans else 0]
    A, T = run[0], 6
    plain = roll(torch, run, T)
    for ext in (False, True):
        link = srbnmpc.LinkModel(seed=4, delay=dev(torch, np.zeros(A, np.int32)), drop=dev(torch, np.zeros(A)),
                                 extrapolate=ext)
        got = roll(torch, run, T, link)
        assert (got["link_age"] == 0).all() and got["link_age"].shape == (T, A)
        # (the final advance rewrote last_state for cycle T; what was seen is cycle T - 1's truth)
        np.testing.assert_array_equal(got["seen_state"], got["traj"][T - 1][:, [0, 2, 1, 3]])
        for k, v in plain.items():
            assert np.array_equal(got[k], v), (ext, k)
    assert not np.array_equal(plain["traj"][T], plain["traj"][0])


def drive(r, T, entry, link=None):
    """T cycles of the Rollout r (after reset) by the C driver called directly."""
    s, o = r.solver, r.out
    r._reserve(T)
    b = srbnmpc.Batch(None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], r.A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, _dp(o["alpha"]), None, 0, None,
                      _dp(o.get("plan")))
    lib = srbnmpc.lib()
    if entry == "plant":
        rc = lib.srb_rollout_plant_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), None, None, None, None, T,
                                          s._stream(None))
    else:
        rc = lib.srb_rollout_link_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), None, None, None, None,
                                         None if link is None else ctypes.byref(link), T, s._stream(None))
    srbnmpc._check(rc)
    r.c, r.flushed = T, True
    return host(r.results())


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_no_link_and_a_struct_of_null_tables_are_the_old_path_bitwise(plans):
    torch = _need_gpu()
    run = sim_oracle.RUNS[1 if plans else 0]
    A, N, C, Ko, Kn, _, _, _ = run
    T = 6
    state, goal, obstacles = team_kw(torch, run)
    _, age = guarded(torch, (T, A), torch.int32)
    _, seen = guarded(torch, (A, 4), torch.float64)
    empty = srbnmpc.Link(99, None, None, None, None, 2, 1, None, None, None, None, None, _dp(seen), None, _ip(age))
    res = []
    for entry, link in (("plant", None), ("link", None), ("link", empty)):
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles))
        r.reset(dev(torch, state))
        res.append(drive(r, T, entry, link))
    assert (age == FILL).all() and (seen == FILL).all() and "link_age" not in res[0]
    for other in res[1:]:
        assert sorted(other) == sorted(res[0])
        for k, v in res[0].items():
            assert np.array_equal(other[k], v), k
    assert not np.array_equal(res[0]["traj"][T], res[0]["traj"][0])


def degraded(torch, A, seed=21, extrapolate=True):
    """Host tables and the LinkModel of the closed-loop tests: every row two cycles late, a fifth of the broadcasts
    lost, positions off by up to 3 cm."""
    tab = link_oracle.tables(seed, np.full(A, 2, np.int32), np.full(A, 0.2), np.full(A, 0.03), None, 2, int(extrapolate))
    model = srbnmpc.LinkModel(seed=seed, delay=dev(torch, tab["delay"]), drop=dev(torch, tab["drop"]),
                              noise_p=dev(torch, tab["noise_p"]), extrapolate=extrapolate)
    return tab, model


@gpu
@pytest.mark.parametrize("extrapolate", [False, True])
def test_closed_loop_every_cycle_from_the_logs(extrapolate):
    run = sim_oracle.RUNS[1]
    A, N, C, Ko, Kn, T, _, plans = run
    torch = _need_gpu()
    state, goal, obstacles = team_kw(torch, run)
    tab, model = degraded(torch, A, extrapolate=extrapolate)
    r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles),
                        link=model)
    r.reset(dev(torch, state))
    cyc = []
    for c in range(T):
        r.step()
        cyc.append({k: getattr(r, k).cpu().numpy() for k in ("last_state", "plan_table", "seen_state", "seen_plan")})
        cyc[-1]["d_agent"] = r.metrics["d_agent"].cpu().numpy()
    res = host(r.results())
    p = sim_oracle.closed_loop(run)["p"]
    st = link_oracle.new_state(A, N, tab["max_delay"])
    m = sim_oracle.Metrics(0)
    worst, differs = 0.0, 0
    for c in range(T):
        b, table = sim_oracle.cycle_inputs(p, res["traj"][c], goal, obstacles, c, res["x"][c - 1] if c else None, plans)
        np.testing.assert_array_equal(cyc[c]["last_state"], b["last_state"], err_msg=f"cycle {c}")
        if c:
            np.testing.assert_array_equal(cyc[c]["plan_table"], table, err_msg=f"cycle {c}")
        seen, seen_plan, age, st = link_oracle.update(c, 0, b["last_state"], table, tab, st)
        np.testing.assert_array_equal(cyc[c]["seen_state"], seen, err_msg=f"cycle {c}")
        np.testing.assert_array_equal(res["link_age"][c], age, err_msg=f"cycle {c}")
        if c:
            np.testing.assert_array_equal(cyc[c]["seen_plan"], seen_plan, err_msg=f"cycle {c}")
        differs += not np.array_equal(seen, b["last_state"])
        m.update(c, res["traj"][c], obstacles, b["last_state"])               # the metrics: the truth
        np.testing.assert_array_equal(cyc[c]["d_agent"], m.d_agent, err_msg=f"cycle {c}")
        b["nbr_state"] = seen                                                   # the solve: what is seen
        o = plan_oracle.solve(p, b, seen_plan)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        worst = max(worst, np.abs(xus(N, res["x"][c]) - xus(N, o["x"])).max())
        np.testing.assert_allclose(xus(N, res["x"][c]), xus(N, o["x"]), atol=NLP_TOL, rtol=0, err_msg=f"cycle {c}")
        np.testing.assert_array_equal(res["traj"][c + 1], sim_oracle.next_state(res["x"][c]), err_msg=f"cycle {c}")
    np.testing.assert_array_equal(res["min_d_agent"], m.min_d_agent)
    np.testing.assert_array_equal(res["min_d_obs"], m.min_d_obs)
    print(f"run {run}, extrapolate {extrapolate}: max |X,U,s - oracle| over {T} cycles = {worst:.3e}; {differs} cycles see "
          f"another table than the truth; largest age {res['link_age'].max()}; min_d_agent {res['min_d_agent'].min():.4f}")
    assert differs >= 1 and res["link_age"].max() >= 2 and (res["link_age"][2:] >= 2).all()


@gpu
def test_c_driver_equals_python_steps_bitwise_with_link_plant_and_plans():
    torch = _need_gpu()
    run = sim_oracle.RUNS[1]
    A, T = run[0], run[5]
    res = []
    for mode in ("run", "step"):
        _, model = degraded(torch, A)
        res.append(roll(torch, run, T, model, mode, plant_seed=21, kick_v=dev(torch, np.full(A, 0.05)),
                        plant_hcom=dev(torch, workload.plant_tables(A, 3)[2])))
    a, b = res
    assert sorted(a) == sorted(b) and {"disturbance", "link_age", "seen_state", "seen_plan"} <= set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["link_age"].max() >= 2 and (a["disturbance"][:, :, 1] != 0).all()
    assert not np.array_equal(a["seen_state"], a["traj"][T - 1][:, [0, 2, 1, 3]])


@gpu
def test_two_shards_reproduce_the_team_bitwise():
    """As test_plant_gpu's shard test, with plans: two shards (cut at 7), each with the whole link tables and a callable
    exchange of the snapshot rows and of the plans, against the whole team's run().  Every shard computes the whole
    perceived table itself."""
    torch = _need_gpu()
    run = sim_oracle.RUNS[1]
    A, N, C, Ko, Kn, _, _, plans = run
    T = 4
    state, goal, obstacles = team_kw(torch, run)
    tab, model = degraded(torch, A)
    want = roll(torch, run, T, model)
    ob = dev(torch, obstacles)
    cut, sh = 7, []
    for lo, hi in ((0, cut), (cut, A)):
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), hi - lo)
        r = srbnmpc.Rollout(s, dev(torch, goal[lo:hi]), plans=plans, log_x=True, obstacles=ob, agent_offset=lo, n_all=A,
                            link=degraded(torch, A)[1])
        r.reset(dev(torch, state[lo:hi]))
        sh.append(r)
    for _ in range(T):
        for r in sh:
            r.advance()
        table = torch.cat([r.last_state for r in sh]).contiguous()
        ptable = torch.cat([r.plan_table for r in sh]).contiguous()
        for r in sh:
            r.step(exchange=lambda local, table=table: table, plan_exchange=lambda local, ptable=ptable: ptable)
    got = [host(r.results()) for r in sh]
    for r in sh:
        np.testing.assert_array_equal(r.seen_state.cpu().numpy(), want["seen_state"])
        np.testing.assert_array_equal(r.seen_plan.cpu().numpy(), want["seen_plan"])
    for k, v in want.items():
        if k in ("seen_state", "seen_plan", "last_state"):
            continue
        if k == "cycles":
            assert got[0][k] == got[1][k] == T
        elif k == "link_age":                                 # the whole table in every shard
            assert np.array_equal(got[0][k], v) and np.array_equal(got[1][k], v)
        else:
            cat = np.concatenate([g[k] for g in got], 1 if v.ndim > 1 and k not in ("state",) else 0)
            assert np.array_equal(cat, v), k
    assert want["link_age"].max() >= 2
    for r in sh:
        r.solver.close()


@gpu
def test_replicas_of_one_scene_draw_by_their_global_rows():
    """workload.replicate_scenes of one 4-agent scene x 8 under set_scenes: with a noise table of zeros every replica is
    the same rollout; with noise_p 0.03 and drop 0.3 every replica has its own draws, the restatement's at its global
    rows; the same seed gives the same bits, another seed another rollout."""
    torch = _need_gpu()
    team, n_obs, copies, N, C, T = 4, 5, 8, 4, 2, 4
    sc = workload.replicate_scenes(workload.make_scenes(1, team, N, C, seed=2, n_obs=n_obs), copies)
    A = team * copies
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=1, K_nbr=2), A)
    s.set_scenes(team, n_obs)

    def go(noise, drop, seed):
        link = srbnmpc.LinkModel(seed=seed, noise_p=dev(torch, np.full(A, noise)), drop=dev(torch, np.full(A, drop)))
        r = srbnmpc.Rollout(s, dev(torch, sc["goal"]), phase=dev(torch, sc["phase"]), log_x=True,
                            obstacles=dev(torch, sc["obstacles"]), link=link)
        r.reset(dev(torch, sc["x0"]))
        r.run(T)
        out = host(r.results())
        out["seen_state"] = r.seen_state.cpu().numpy()
        out["scenes"] = host(r.scene_results())
        return out
    calm = go(0.0, 0.0, 5)
    per = calm["traj"].reshape(T + 1, copies, team, 4)
    assert (calm["link_age"] == 0).all() and (per == per[:, :1]).all()
    a, again, other = go(0.03, 0.3, 5), go(0.03, 0.3, 5), go(0.03, 0.3, 6)
    for k in a:
        if k != "scenes":
            assert np.array_equal(a[k], again[k]), k
    assert not np.array_equal(a["seen_state"], other["seen_state"]) and not np.array_equal(a["link_age"], other["link_age"])
    tab = link_oracle.tables(5, None, np.full(A, 0.3), np.full(A, 0.03), None, 0, 0)
    truth = a["traj"][:T][:, :, [0, 2, 1, 3]]
    want = link_oracle.run(0, truth, None, tab, N)
    for c in range(T):
        np.testing.assert_array_equal(a["link_age"][c], want[c][2])
    np.testing.assert_array_equal(a["seen_state"], want[T - 1][0])
    err = (want[T - 1][0] - np.where((want[T - 1][2] == 0)[:, None], truth[T - 1], np.nan)).reshape(copies, team, 4)[..., :2]
    for i in range(copies):                                   # the fresh rows' errors differ between replicas
        for j in range(i):
            both = ~np.isnan(err[i]) & ~np.isnan(err[j])
            assert (err[i][both] != err[j][both]).all(), (i, j)
    ages = a["link_age"].reshape(T, copies, team)
    assert any(not np.array_equal(ages[:, i], ages[:, 0]) for i in range(1, copies))
    assert a["scenes"]["n_scenes"] == copies and a["scenes"]["min_d_agent"].shape == (copies,)
    s.close()


@gpu
def test_refusals_by_name_on_a_live_context_and_it_survives():
    torch = _need_gpu()
    run = sim_oracle.RUNS[2]
    A, N, C, Ko, Kn, T, seed, plans = run
    state, goal, obstacles = team_kw(torch, run)
    s = solver(N, C, Ko, Kn)
    tab, model = degraded(torch, A)
    r = srbnmpc.Rollout(s, dev(torch, goal), plans=True, log_x=True, obstacles=dev(torch, obstacles), link=model)
    r.reset(dev(torch, state))
    r._reserve(2)
    lib = srbnmpc.lib()
    err = lambda: lib.srb_last_error().decode()
    o = r.out
    b = srbnmpc.Batch(None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, _dp(o["x"]), _dp(o["obj"]),
                      _ip(o["status"]), _ip(o["iters"]), None, _dp(o["alpha"]), None, 0, None, _dp(o["plan"]))

    def rollout_rc(link, batch=b):
        return lib.srb_rollout_link_device(s._h, A, ctypes.byref(batch), ctypes.byref(r._sim()), None, None, None, None,
                                           ctypes.byref(link), 1, s._stream(None))

    def update_rc(link, plan=r.plan_table):
        return lib.srb_link_update_device(s._h, A, ctypes.byref(link), _dp(r.last_state), _dp(plan), 1, 0, s._stream(None))
    # the horizon-aware plan selection reads the agent's own row of the table
    s.set_option("plan_selection", 1)
    try:
        assert rollout_rc(r._link()) == -1 and "SRB_OPT_PLAN_SELECTION = 1 with a srb_link" in err()
        assert update_rc(r._link()) == -1 and "SRB_OPT_PLAN_SELECTION = 1 with a srb_link" in err()
    finally:
        s.set_option("plan_selection", 0)
    # a shard cannot roll out alone, link or not
    shard = srbnmpc.Batch.from_buffer_copy(b)
    shard.agent_offset = 1
    assert rollout_rc(r._link(), shard) == -1 and "sharded" in err()
    # overlapping buffers
    for name, other, word, both in (("seen_state", r.last_state, "srb_link.seen_state overlaps last_state", True),
                                    ("seen_plan", r.plan_table, "srb_link.seen_plan overlaps plan_table", True),
                                    ("seen_plan", o["plan"], "srb_link.seen_plan overlaps srb_batch.plan", False)):
        link = r._link()
        setattr(link, name, _dp(other))
        assert rollout_rc(link) == -1 and word in err(), (word, err())
        if both:
            assert update_rc(link) == -1 and word in err(), (word, err())
    # the Python layer, by name
    z = np.zeros(A)
    for kw, word in ((dict(delay=dev(torch, np.full(A, 17, np.int32))), "link: delay must be 0 .. 16"),
                     (dict(delay=dev(torch, np.full(A, -1, np.int32))), "link: delay must be 0 .. 16"),
                     (dict(delay=dev(torch, np.zeros(A))), "link: delay"),
                     (dict(delay=dev(torch, np.zeros(A + 1, np.int32))), "link: delay"),
                     (dict(drop=dev(torch, z + 1.5)), "link: drop must be <= 1"),
                     (dict(drop=dev(torch, z - 0.1)), "link: drop must be >= 0"),
                     (dict(noise_p=dev(torch, z - 0.1)), "link: noise_p must be >= 0"),
                     (dict(noise_v=dev(torch, z + np.nan)), "link: noise_v must be finite"),
                     (dict(noise_v=z), "link: noise_v"), (dict(seed=-1, drop=dev(torch, z)), "link: seed")):
        with pytest.raises(ValueError, match=word):
            srbnmpc.Rollout(s, dev(torch, goal), obstacles=dev(torch, obstacles), link=srbnmpc.LinkModel(**kw))
    with pytest.raises(ValueError, match="link must be a srbnmpc.LinkModel"):
        srbnmpc.Rollout(s, dev(torch, goal), obstacles=dev(torch, obstacles), link=dict(delay=None))
    # after the refusals a plain rollout on the same context gives the bits it always gave
    plain = srbnmpc.Rollout(s, dev(torch, goal), plans=True, log_x=True, obstacles=dev(torch, obstacles))
    plain.reset(dev(torch, state))
    plain.run(T)
    res = host(plain.results())
    want = trg.rollout(run)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
