"""GPU tests of the closed-loop rollout (csrc/srb_sim.hip, srb_rollout_device, srbnmpc.Rollout).

The two kernels are compared bit for bit with their numpy restatement (tests/sim_oracle.py).  The closed loop is
checked per cycle, so that nothing drifts: the inputs of every cycle are rebuilt from the device's own logged state
by the restatement and solved by the plan oracle, to the tolerances of tests/test_gpu_parity.py (statuses exact;
X, U, s within NLP_TOL = 1e-4), and the next logged state is the gather of the logged solution, bitwise."""
import ctypes

import numpy as np
import pytest

import plan_oracle
import sim_oracle
import srbnmpc
from srbnmpc import workload

NLP_TOL = 1e-4
gpu = pytest.mark.gpu
TS = workload.TS


def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, C, Ko, Kn, max_agents=320):
    key = (N, C, Ko, Kn, max_agents)
    if key not in _solvers:
        _solvers[key] = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), max_agents)
    return _solvers[key]


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


# ================================================================================== 1. the kernels, bitwise
@gpu
@pytest.mark.parametrize("A,N,C,n_obs,with_phase", [(5, 4, 2, 0, False), (300, 10, 2, 300, True), (300, 4, 4, 300, False),
                                                    (5, 10, 4, 300, True)])
def test_kernels_equal_the_restatement_bitwise(A, N, C, n_obs, with_phase):
    """Both kernels through the C entry points, at a first cycle (the caller's state) and at a later one (the
    state, the shifted plans and the logs from a decision vector x): every output array against numpy.
    A = 300 is a partial second block and n_all = 300 / n_obs = 300 a tile remainder; agents 0 and 1 are the
    arrival cases, the later cycle's snapshot row 2 holds a NaN (its state came from a NaN in x), and the obstacles are
    sparse enough that agents are inside 0.5 m at the first cycle, first at the later one, and never."""
    torch = _need_gpu()
    s = solver(N, C, 1, 0)
    p, nv = s.params, s.params.nv
    rng = np.random.default_rng(A + N + C)
    state = np.stack([rng.uniform(0, 9, A), rng.uniform(-.3, .3, A), rng.uniform(-2, 2, A), rng.uniform(-.3, .3, A)], 1)
    goal = np.tile([10.0, 0.0], (A, 1))
    state[0, [1, 3]] = 0.0; goal[0] = state[0, [0, 2]]
    state[1, [1, 3]] = 0.0; goal[1] = state[1, [0, 2]] + [0.03, 0.02]
    phase = rng.integers(0, 4, A).astype(np.int32) if with_phase else None
    obstacles = np.stack([rng.uniform(0, 60, n_obs), rng.uniform(-20, 20, n_obs)], 1)
    x = rng.normal(size=(A, nv)); x[:, 12] = rng.uniform(0, 9, A); x[:, 14] = rng.uniform(-2, 2, A)
    x[2, 12] = np.nan                                        # a NaN state travels into snapshot row 2 at cycle c1
    status = rng.integers(0, 5, (A, 2)).astype(np.int32); iters = rng.integers(0, 50, (A, 2)).astype(np.int32)
    c0, c1 = 3, 6
    f8, i4 = torch.float64, torch.int32
    z = lambda *sh, dt=f8: torch.full(sh, -7, dtype=dt, device="cuda")
    t = dict(state=dev(torch, state), goal=dev(torch, goal), phase=None if phase is None else dev(torch, phase),
             x=dev(torch, x), status=dev(torch, status), iters=dev(torch, iters), x0=z(A, 4), ref=z(A, 4 * N),
             foot=z(A, N, 2, C), last_state=z(A, 4), alpha_buf=z(A, 4), plan_table=z(A, N, 2), traj=z(c1 - c0 + 1, A, 4),
             status_log=z(c1 - c0, A, 2, dt=i4), iters_log=z(c1 - c0, A, 2, dt=i4), x_log=z(c1 - c0, A, nv),
             obstacles=dev(torch, obstacles) if n_obs else None, d_obs=z(A), d_agent=z(A), min_d_obs=z(A),
             min_d_agent=z(A), fail_cycle=z(A, dt=i4), distance_to_fail=z(A))
    dp = lambda k: None if t[k] is None else ctypes.cast(ctypes.c_void_p(t[k].data_ptr()), srbnmpc._dp)
    ip = lambda k: None if t[k] is None else ctypes.cast(ctypes.c_void_p(t[k].data_ptr()), srbnmpc._ip)
    sim = srbnmpc.Sim(dp("state"), dp("goal"), ip("phase"), 0.27, c0, dp("x"), ip("status"), ip("iters"), dp("x0"),
                      dp("ref"), dp("foot"), dp("last_state"), dp("alpha_buf"), dp("plan_table"), dp("traj"),
                      ip("status_log"), ip("iters_log"), dp("x_log"), dp("obstacles"), dp("last_state"), n_obs, A, 0,
                      dp("d_obs"), dp("d_agent"), dp("min_d_obs"), dp("min_d_agent"), ip("fail_cycle"),
                      dp("distance_to_fail"))
    lib, st = srbnmpc.lib(), s._stream(None)
    m = sim_oracle.Metrics(c0)
    want_state = state
    for c in (c0, c1):
        srbnmpc._check(lib.srb_sim_advance_device(s._h, A, ctypes.byref(sim), c, st))
        srbnmpc._check(lib.srb_sim_metrics_device(s._h, A, ctypes.byref(sim), c, st))
        torch.cuda.synchronize()
        got = {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}
        if c == c1:
            want_state = sim_oracle.next_state(x)
        w = sim_oracle.advance(N, C, TS, want_state, goal, 0.27, c, phase)
        m.update(c, want_state, obstacles, w["last_state"])
        for k in ("x0", "ref", "foot", "last_state"):
            assert np.array_equal(got[k], w[k], equal_nan=True), (c, k)
        assert np.array_equal(got["state"], want_state, equal_nan=True) and np.array_equal(got["alpha_buf"], want_state, equal_nan=True)
        assert np.array_equal(got["traj"][c - c0], want_state, equal_nan=True)
        for k, v in m.as_dict().items():
            assert np.array_equal(got[k], v, equal_nan=True), (c, k, got[k][:6], v[:6])
        if c == c0:                                          # nothing of a previous solve is written at c_first
            assert (got["plan_table"] == -7).all() and (got["status_log"] == -7).all() and (got["x_log"] == -7).all()
        else:
            r = c - c0 - 1
            assert np.array_equal(got["plan_table"], sim_oracle.shift4(N, x), equal_nan=True)
            assert np.array_equal(got["status_log"][r], status) and np.array_equal(got["iters_log"][r], iters)
            assert np.array_equal(got["x_log"][r], x, equal_nan=True)
            assert (got["x_log"][:r] == -7).all() and (got["traj"][1:c - c0] == -7).all()
    assert np.isfinite(got["ref"][[0, 1, 3]]).all()
    if n_obs and A == 300:
        assert (m.fail_cycle == c0).any() and (m.fail_cycle == c1).any() and (m.fail_cycle < 0).any()
    if not n_obs:
        assert np.isinf(got["d_obs"]).all() and (got["fail_cycle"] == -1).all()
    assert np.isinf(got["d_agent"][2]) and np.isfinite(np.delete(got["d_agent"], 2)).all()   # the NaN row never wins


# ================================================================================== the closed loop
_rolls = {}


def rollout(run, mode="run"):
    """One of sim_oracle.RUNS on the device with log_x, computed once per (run, mode): the host copies of
    results() plus the plans flag.  mode "run": the C driver; "step": T x step()."""
    if (run, mode) not in _rolls:
        torch = _need_gpu()
        A, N, C, Ko, Kn, T, seed, plans = run
        state, goal, obstacles = sim_oracle.team(A, N, C, seed)
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=dev(torch, obstacles))
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        _rolls[(run, mode)] = host(r.results())
    return _rolls[(run, mode)]


@gpu
@pytest.mark.parametrize("run", sim_oracle.RUNS)
def test_every_cycle_matches_the_oracle_on_the_logged_state(run):
    A, N, C, Ko, Kn, T, seed, plans = run
    res = rollout(run)
    R = sim_oracle.closed_loop(run)
    p = R["p"]
    assert res["cycles"] == T and res["traj"].shape == (T + 1, A, 4) and res["x"].shape == (T, A, (6 + C) * N + 1)
    assert np.array_equal(res["traj"][0], R["state0"])
    worst = 0.0
    for c in range(T):
        b, table = sim_oracle.cycle_inputs(p, res["traj"][c], R["goal"], R["obstacles"], c, res["x"][c - 1] if c else None, plans)
        o = plan_oracle.solve(p, b, table)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        e = np.abs(xus(N, res["x"][c]) - xus(N, o["x"])).max()
        worst = max(worst, e)
        np.testing.assert_allclose(xus(N, res["x"][c]), xus(N, o["x"]), atol=NLP_TOL, rtol=0, err_msg=f"cycle {c}")
        assert np.array_equal(res["traj"][c + 1], sim_oracle.next_state(res["x"][c])), c
    assert np.array_equal(res["state"], res["traj"][T])
    sep_dev, sep_orc = res["min_d_agent"].min(), R["metrics"]["min_d_agent"].min()
    print(f"run {run}: max |X,U,s - oracle| over {T} cycles = {worst:.3e}; final separation device {sep_dev:.6f} "
          f"oracle-only {sep_orc:.6f}; min_d_obs device {res['min_d_obs'].min():.6f} oracle-only "
          f"{R['metrics']['min_d_obs'].min():.6f}")


@gpu
@pytest.mark.parametrize("run", [sim_oracle.RUNS[1], sim_oracle.RUNS[3]])
def test_c_driver_equals_python_steps_bitwise(run):
    a, b = rollout(run, "run"), rollout(run, "step")
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@gpu
def test_shards_reproduce_the_full_team_bitwise():
    """Two Rollout objects on shards of the 16-agent team (agent_offset, the all-gather stood in for by torch.cat
    of the two snapshots) against the full-team rollout, 3 cycles."""
    torch = _need_gpu()
    run = sim_oracle.RUNS[0]
    A, N, C, Ko, Kn, T, seed, plans = run
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    ob = dev(torch, obstacles)
    full = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), log_x=True, obstacles=ob)
    full.reset(dev(torch, state))
    full.run(3)
    want = host(full.results())
    cut = 7
    sh = []
    for lo, hi in ((0, cut), (cut, A)):
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), hi - lo)
        r = srbnmpc.Rollout(s, dev(torch, goal[lo:hi]), log_x=True, obstacles=ob, agent_offset=lo, n_all=A)
        r.reset(dev(torch, state[lo:hi]))
        sh.append(r)
    with pytest.raises(ValueError, match="exchange"):
        sh[1].step()
    with pytest.raises(ValueError, match="whole team"):
        sh[1].run(1)
    for _ in range(3):
        for r in sh:                                       # every shard's snapshot rows, then the "all-gather"
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
@pytest.mark.parametrize("run", [sim_oracle.RUNS[0], sim_oracle.RUNS[2]])
def test_fail_cycle_and_metrics_equal_the_restatement(run):
    """The six metric arrays from the device's own trajectory, replayed through the restatement; run 2 holds the
    crossing at cycle 5, run 0 the agents inside 0.5 m from the start and the ones that never are."""
    A, N, C, Ko, Kn, T, seed, plans = run
    res = rollout(run)
    R = sim_oracle.closed_loop(run)
    m = sim_oracle.Metrics(0)
    for c in range(T):
        st = res["traj"][c]
        m.update(c, st, R["obstacles"], np.stack([st[:, 0], st[:, 2], st[:, 1], st[:, 3]], 1))
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)
    fc = res["fail_cycle"]
    if N == 4:
        assert (fc == 5).sum() == 1 and (fc[fc > 0] == 5).all()
        a = int(np.argmax(fc == 5))
        assert res["distance_to_fail"][a] == np.sqrt(res["traj"][5, a, 0] ** 2 + res["traj"][5, a, 2] ** 2)
    else:
        assert 5 <= (fc == 0).sum() <= 6 and (fc < 0).any()
    assert (res["distance_to_fail"][fc < 0] == 0).all()


@gpu
def test_refusals_by_name_and_the_context_survives():
    torch = _need_gpu()
    run = sim_oracle.RUNS[2]
    A, N, C, Ko, Kn, T, seed, plans = run
    state, goal, obstacles = sim_oracle.team(A, N, C, seed)
    s = solver(N, C, Ko, Kn)
    r = srbnmpc.Rollout(s, dev(torch, goal), plans=True, log_x=True, obstacles=dev(torch, obstacles))
    lib = srbnmpc.lib()
    err = lambda: lib.srb_last_error().decode()
    with pytest.raises(RuntimeError, match="reset"):
        r.run(1)
    r.reset(dev(torch, state))
    r._reserve(2)
    o = r.out
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)

    def batch(**kw):
        b = srbnmpc.Batch(None, None, None, dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, dp(o["x"]), dp(o["obj"]),
                          ip(o["status"]), ip(o["iters"]), None, dp(o["alpha"]), None, 0, None, dp(o["plan"]))
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    call = lambda b, sim, n=A: lib.srb_rollout_device(s._h, n, ctypes.byref(b), ctypes.byref(sim), 1, s._stream(None))
    assert call(batch(agent_offset=1), r._sim()) == -1 and "sharded" in err()
    assert call(batch(n_all=A + 1), r._sim()) == -1 and "sharded" in err()
    sim = r._sim(); sim.plan_table = dp(o["plan"])
    assert call(batch(), sim) == -1 and "overlaps" in err()
    sim = r._sim(); sim.x = None
    assert lib.srb_sim_advance_device(s._h, A, ctypes.byref(sim), 1, s._stream(None)) == -1 and "srb_sim.x" in err()
    s2 = srbnmpc.BatchSolver(srbnmpc.default_params(3, 2), 4)
    assert lib.srb_sim_advance_device(s2._h, 4, ctypes.byref(r._sim()), 0, s2._stream(None)) == -1 and "N >= 4" in err()
    with pytest.raises(ValueError, match="N >= 4"):
        srbnmpc.Rollout(s2, dev(torch, goal[:4]))
    s2.close()
    with pytest.raises(ValueError, match="goal"):
        srbnmpc.Rollout(s, dev(torch, goal).float())
    with pytest.raises(ValueError, match="state"):
        r.reset(dev(torch, state)[:, :3])
    # after the refusals the same object rolls out as if nothing had happened
    r.reset(dev(torch, state))
    r.run(T)
    res = host(r.results())
    want = rollout(run)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
