"""GPU tests of the SRB-12 closed-loop rollout and scene batching (csrc/srb12_sim.hip, srb12_rollout_device,
srb12_ctx_set_scenes, srb12.Rollout12).

The advance kernel is compared with its numpy restatement (tests/sim12_oracle.py): bitwise, except the arrays that
pass through atan2 / cos / sin, which agree within sim12_oracle.TRIG_TOL.  The closed loop is checked per cycle, so
that nothing drifts: the inputs of every cycle are rebuilt from the device's own logged state by the restatement
and solved by oracle.solve_batch12, to the bounds of tests/test_srb12.py (statuses exact; X within 1e-6, forces
within 1e-4 N, s within 1e-6), and the next logged state is the gather of the logged solution, bitwise."""
import ctypes

import numpy as np
import pytest
from conftest import converged

import sim12_oracle
import sim_oracle
import srbnmpc
from srbnmpc import rollout, srb12, workload

gpu = pytest.mark.gpu
TS = workload.TS
X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_srb12.py


def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, Ko, Kn, max_agents=320):
    key = (N, Ko, Kn, max_agents)
    if key not in _solvers:
        _solvers[key] = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), max_agents)
    return _solvers[key]


def dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def kernel_case(A, N, n_obs):
    """Inputs of test_kernels_equal_the_restatement (numpy only): states in the reference's arena with yaws beyond
    +-pi, agents 0 and 1 the arrival cases, agent 3's goal behind it, sparse obstacles, and a decision vector whose
    X at grid index 3 is a state of the same kind with a NaN in agent 2's x."""
    rng = np.random.default_rng(A + N + n_obs)

    def states():
        st = rng.normal(size=(A, 12)) * 0.05
        st[:, 0] = rng.uniform(0, 9, A); st[:, 1] = rng.uniform(-2, 2, A); st[:, 2] += 0.3
        st[:, 5] = rng.uniform(-4, 4, A); st[:, 6:8] = rng.uniform(-.3, .3, (A, 2))
        return st
    state = states()
    goal = np.tile([10.0, 0.0], (A, 1))
    state[0, 6:12] = 0.0; goal[0] = state[0, :2]
    state[1, 6:12] = 0.0; goal[1] = state[1, :2] + [0.03, 0.0]
    goal[3] = state[3, :2] - [3.0, 1.0]
    phase = rng.integers(0, 4, A).astype(np.int32)
    obstacles = np.stack([rng.uniform(0, 60, n_obs), rng.uniform(-20, 20, n_obs)], 1)
    nv = 24 * N + 1
    x = rng.normal(size=(A, nv))
    x[:, 36:48] = states()
    x[2, 36] = np.nan
    status = rng.integers(0, 5, (A, 2)).astype(np.int32); iters = rng.integers(0, 50, (A, 2)).astype(np.int32)
    return dict(state=state, goal=goal, phase=phase, obstacles=obstacles, x=x, status=status, iters=iters)


def assert_advance_equal(got, w, where):
    """Every output of the advance against the restatement: bitwise, except xref column 5 and foot x, y
    (sim12_oracle.TRIG_TOL).  Returns the largest difference found in those."""
    for k in ("x0", "last_state", "com", "contact"):
        assert np.array_equal(got[k], w[k], equal_nan=True), (where, k)
    plain = [i for i in range(12) if i != 5]
    assert np.array_equal(got["xref"][:, :, plain], w["xref"][:, :, plain], equal_nan=True), (where, "xref")
    assert np.array_equal(got["foot"][:, :, :, 2], w["foot"][:, :, :, 2]), (where, "foot z")
    worst = 0.0
    for g, v, name in ((got["xref"][:, :, 5], w["xref"][:, :, 5], "yaw_ref"), (got["foot"][:, :, :, :2], w["foot"][:, :, :, :2], "foot")):
        assert np.array_equal(np.isnan(g), np.isnan(v)), (where, name)
        np.testing.assert_allclose(g, v, rtol=0, atol=sim12_oracle.TRIG_TOL, equal_nan=True, err_msg=f"{where} {name}")
        worst = max(worst, np.nanmax(np.abs(g - v)))
    return worst


# ================================================================================== 1. the kernels
@gpu
@pytest.mark.parametrize("A,N,gait,n_obs,with_phase", [(5, 4, "trot", 0, False), (300, 10, "trot", 300, True),
                                                       (300, 4, "stand", 300, False), (5, 10, "stand", 300, True)])
def test_kernels_equal_the_restatement(A, N, gait, n_obs, with_phase):
    """Advance and metrics through the C entry points, at a first cycle (the caller's state) and at a later one (the
    state and the logs from a decision vector x).  A = 300 with N = 10 is 3000 threads, a partial last block whose
    agents straddle blocks; n_all = 300 / n_obs = 300 a tile remainder of the scan.  The later cycle's agent 2 holds
    a NaN (its state came from a NaN in x): it never wins a minimum."""
    torch = _need_gpu()
    s = solver(N, 1, 0)
    nv = s.params.nv
    k = kernel_case(A, N, n_obs)
    state, goal, obstacles, x, status, iters = (k[n] for n in ("state", "goal", "obstacles", "x", "status", "iters"))
    phase = k["phase"] if with_phase else None
    c0, c1 = 3, 6
    f8, i4 = torch.float64, torch.int32
    z = lambda *sh, dt=f8: torch.full(sh, -7, dtype=dt, device="cuda")
    t = dict(state=dev(torch, state), goal=dev(torch, goal), phase=None if phase is None else dev(torch, phase),
             x=dev(torch, x), status=dev(torch, status), iters=dev(torch, iters), x0=z(A, 12), xref=z(A, N, 12),
             foot=z(A, N, 4, 3), contact=z(A, N, 4, dt=i4), last_state=z(A, 4), com=z(A, 4), traj=z(c1 - c0 + 1, A, 12),
             status_log=z(c1 - c0, A, 2, dt=i4), iters_log=z(c1 - c0, A, 2, dt=i4), x_log=z(c1 - c0, A, nv),
             obstacles=dev(torch, obstacles) if n_obs else None, d_obs=z(A), d_agent=z(A), min_d_obs=z(A),
             min_d_agent=z(A), fail_cycle=z(A, dt=i4), distance_to_fail=z(A))
    dp = lambda n: None if t[n] is None else ctypes.cast(ctypes.c_void_p(t[n].data_ptr()), srbnmpc._dp)
    ip = lambda n: None if t[n] is None else ctypes.cast(ctypes.c_void_p(t[n].data_ptr()), srbnmpc._ip)
    sim = srb12.Sim12(dp("state"), dp("goal"), ip("phase"), 0.27, 0.3, 0.1, 0.05, srb12.GAITS[gait], c0, dp("x"),
                      ip("status"), ip("iters"), dp("x0"), dp("xref"), dp("foot"), ip("contact"), dp("last_state"),
                      dp("com"), dp("traj"), ip("status_log"), ip("iters_log"), dp("x_log"), dp("obstacles"),
                      dp("last_state"), n_obs, A, 0, dp("d_obs"), dp("d_agent"), dp("min_d_obs"), dp("min_d_agent"),
                      ip("fail_cycle"), dp("distance_to_fail"))
    lib, st = srb12._lib(), s._stream(None)
    m = sim_oracle.Metrics(c0)
    want_state = state
    worst = 0.0
    for c in (c0, c1):
        srbnmpc._check(lib.srb12_sim_advance_device(s._h, A, ctypes.byref(sim), c, st))
        srbnmpc._check(lib.srb12_sim_metrics_device(s._h, A, ctypes.byref(sim), c, st))
        torch.cuda.synchronize()
        got = {n: (None if v is None else v.cpu().numpy()) for n, v in t.items()}
        if c == c1:
            want_state = sim12_oracle.next_state12(x)
        w = sim12_oracle.advance12(N, TS, want_state, goal, 0.27, c, phase, gait)
        m.update(c, w["com"], obstacles, w["last_state"])
        worst = max(worst, assert_advance_equal(got, w, c))
        assert np.array_equal(got["state"], want_state, equal_nan=True)
        assert np.array_equal(got["traj"][c - c0], want_state, equal_nan=True)
        for n, v in m.as_dict().items():
            assert np.array_equal(got[n], v, equal_nan=True), (c, n, got[n][:6], v[:6])
        if c == c0:                                          # nothing of a previous solve is written at c_first
            assert (got["status_log"] == -7).all() and (got["iters_log"] == -7).all() and (got["x_log"] == -7).all()
            assert (got["traj"][1:] == -7).all()
        else:
            r = c - c0 - 1
            assert np.array_equal(got["status_log"][r], status) and np.array_equal(got["iters_log"][r], iters)
            assert np.array_equal(got["x_log"][r], x, equal_nan=True)
            assert (got["x_log"][:r] == -7).all() and (got["traj"][1:c - c0] == -7).all()
    print(f"case {(A, N, gait, n_obs, with_phase)}: max |device - numpy| of the trig-derived outputs {worst:.3e}")
    assert np.isfinite(got["xref"][[0, 1, 3]]).all() and np.isfinite(got["foot"][[0, 1, 3]]).all()
    assert np.isnan(got["xref"][2, :, 0]).all() and np.isfinite(got["xref"][2, :, 5]).all()
    if not n_obs:
        assert np.isinf(got["d_obs"]).all() and (got["fail_cycle"] == -1).all()
    else:
        assert np.isinf(got["d_obs"][2]) and np.isfinite(np.delete(got["d_obs"], 2)).all()
    assert np.isinf(got["d_agent"][2]) and np.isfinite(np.delete(got["d_agent"], 2)).all()   # the NaN row never wins


# ================================================================================== the closed loop
_rolls = {}


def rollout12(run, mode="run"):
    """One of sim12_oracle.RUNS12 on the device with log_x, computed once per (run, mode): the host copies of
    results().  mode "run": the C driver; "step": T x step()."""
    if (run, mode) not in _rolls:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = run
        state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
        r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                            obstacles=dev(torch, obstacles))
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = r.results()
        torch.cuda.synchronize()
        _rolls[(run, mode)] = host(res)
    return _rolls[(run, mode)]


@gpu
@pytest.mark.parametrize("run", sim12_oracle.RUNS12)
def test_every_cycle_matches_the_oracle_on_the_logged_state(run):
    A, N, gait, seed, T, Ko, Kn = run
    res = rollout12(run)
    R = sim12_oracle.closed_loop12(run)
    p = R["p"]
    assert res["cycles"] == T and res["traj"].shape == (T + 1, A, 12) and res["x"].shape == (T, A, 24 * N + 1)
    assert np.array_equal(res["traj"][0], R["state0"])
    ex = eu = es = 0.0
    compared = 0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], R["goal"], R["obstacles"], c, R["phase"], gait)
        o = sim12_oracle.solve12(p, b)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        both = converged(res["status"][c]) & converged(o["status"])
        compared += int(both.sum())
        g, w = res["x"][c][both], o["x"][both]
        if both.any():
            ex = max(ex, np.abs(g[:, :12 * N] - w[:, :12 * N]).max())
            eu = max(eu, np.abs(g[:, 12 * N:24 * N] - w[:, 12 * N:24 * N]).max())
            es = max(es, np.abs(g[:, -1] - w[:, -1]).max())
        assert np.array_equal(res["traj"][c + 1], res["x"][c][:, 36:48]), c
    z = res["traj"][:, :, 2]
    print(f"run {run}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; height "
          f"{z.min():.4f} .. {z.max():.4f}; final separation device {res['min_d_agent'].min():.6f} oracle-only "
          f"{R['metrics']['min_d_agent'].min():.6f}; min_d_obs device {res['min_d_obs'].min():.6f} oracle-only "
          f"{R['metrics']['min_d_obs'].min():.6f}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    assert np.array_equal(res["state"], res["traj"][T])


@gpu
@pytest.mark.parametrize("run", [sim12_oracle.RUNS12[0], sim12_oracle.RUNS12[1]])
def test_c_driver_equals_python_steps_bitwise(run):
    a, b = rollout12(run, "run"), rollout12(run, "step")
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("run", [sim12_oracle.RUNS12[0], sim12_oracle.RUNS12[2]])
def test_metrics_equal_the_restatement(run):
    """The six metric arrays from the device's own trajectory, replayed through sim_oracle.Metrics on the com rows."""
    A, N, gait, seed, T, Ko, Kn = run
    res = rollout12(run)
    R = sim12_oracle.closed_loop12(run)
    m = sim_oracle.Metrics(0)
    for c in range(T):
        st = res["traj"][c]
        m.update(c, sim12_oracle.com_of(st), R["obstacles"], st[:, [0, 1, 6, 7]])
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)
    fc = res["fail_cycle"]
    assert (fc == 0).any() and (fc < 0).any()              # inside 0.5 m of an obstacle from the start, and never
    assert (res["distance_to_fail"][fc < 0] == 0).all()
    a = int(np.argmax(fc == 0))
    assert res["distance_to_fail"][a] == np.sqrt(res["traj"][0, a, 0] ** 2 + res["traj"][0, a, 1] ** 2)


# ================================================================================== scenes
S_, TEAM, NOBS, NS = 3, 4, 5, 10


def scene_solver():
    return solver(NS, 3, 8, 12)


def _solve(s, b, rows=slice(None), obs=slice(None)):
    return s.solve(b["x0"][rows], b["xref"][rows], b["foot"][rows], b["contact"][rows], b["obstacles"][obs],
                   b["nbr_state"][rows])


def _roll(torch, s, b, rows=slice(None), obs=slice(None), T=4):
    r = srb12.Rollout12(s, dev(torch, b["goal"][rows]), phase=dev(torch, b["phase"][rows]), log_x=True,
                        obstacles=dev(torch, b["obstacles"][obs]))
    r.reset(dev(torch, b["x0"][rows]))
    r.run(T)
    return r


@gpu
def test_scene_batched_solve_equals_the_per_team_solves_bitwise():
    """3 scenes x 4 agents x 5 obstacles with K 3 + 8, which clamps to 3 + 3.  Setting the scenes back to (0, 0)
    restores the unpartitioned results."""
    _need_gpu()
    b = workload.make_scenes12(S_, TEAM, NS, "trot", seed=11, n_obs=NOBS)
    s = scene_solver()
    assert s.scenes == (0, 0)
    flat = _solve(s, b)
    assert flat["sel"].shape == (S_ * TEAM, 3 + 8)
    teams = [_solve(s, b, slice(i * TEAM, (i + 1) * TEAM), slice(i * NOBS, (i + 1) * NOBS)) for i in range(S_)]
    s.set_scenes(TEAM, NOBS)
    try:
        assert s.scenes == (TEAM, NOBS)
        out = _solve(s, b)
    finally:
        s.set_scenes(0, 0)
    assert out["sel"].shape == (S_ * TEAM, 3 + 3)
    for i, t in enumerate(teams):
        r = slice(i * TEAM, (i + 1) * TEAM)
        assert t["sel"].shape == (TEAM, 3 + 3)
        for k in ("x", "x_qp", "status", "iters", "obj"):
            assert np.array_equal(out[k][r], t[k]), (i, k)
        sel = t["sel"].copy()
        sel[:, :3] = np.where(sel[:, :3] >= 0, sel[:, :3] + i * NOBS, sel[:, :3])
        sel[:, 3:] = np.where(sel[:, 3:] >= 0, sel[:, 3:] + i * TEAM, sel[:, 3:])
        assert np.array_equal(out["sel"][r], sel), (i, out["sel"][r], sel)
    assert not np.array_equal(out["x"], flat["x"])          # the partition matters: other teams are no neighbours
    again = _solve(s, b)
    for k in flat:
        assert np.array_equal(again[k], flat[k]), k


@gpu
def test_scene_batched_rollout_equals_the_per_team_rollouts_bitwise():
    torch = _need_gpu()
    b = workload.make_scenes12(S_, TEAM, NS, "trot", seed=11, n_obs=NOBS)
    s = scene_solver()
    teams = []
    for i in range(S_):
        r = _roll(torch, s, b, slice(i * TEAM, (i + 1) * TEAM), slice(i * NOBS, (i + 1) * NOBS))
        res = r.results(); torch.cuda.synchronize()
        teams.append(host(res))
    s.set_scenes(TEAM, NOBS)
    try:
        r = _roll(torch, s, b)
        res = r.results()
        sc = r.scene_results()
        torch.cuda.synchronize()
        got, sc = host(res), host(sc)
    finally:
        s.set_scenes(0, 0)
    for k, v in got.items():
        if k == "cycles":
            assert v == 4 == teams[0][k]
            continue
        cat = np.concatenate([t[k] for t in teams], 1 if v.ndim > 1 and k != "state" else 0)
        assert np.array_equal(v, cat), k
    want = rollout.reduce_scenes({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in got.items()}, TEAM)
    assert sorted(sc) == sorted(want)
    for k, v in want.items():
        assert np.array_equal(sc[k], v.numpy() if hasattr(v, "numpy") else v), k
    assert sc["n_scenes"] == S_ and sc["scene_agents"] == TEAM
    for i, t in enumerate(teams):
        assert sc["min_d_agent"][i] == t["min_d_agent"].min() and sc["min_d_obs"][i] == t["min_d_obs"].min()
    with pytest.raises(ValueError, match="scene partition"):
        r.scene_results()


# ================================================================================== refusals
@gpu
def test_refusals_by_name_and_the_context_survives():
    torch = _need_gpu()
    run = sim12_oracle.RUNS12[2]
    A, N, gait, seed, T, Ko, Kn = run
    want = rollout12(run)
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    s = solver(N, Ko, Kn)
    r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, obstacles))
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    with pytest.raises(RuntimeError, match="reset"):
        r.run(1)
    r.reset(dev(torch, state))
    r._reserve(2)
    o = r.out
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
    st = s._stream(None)

    def batch(**kw):
        b = srb12.Batch12(None, None, None, None, dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, dp(o["x"]),
                          dp(o["obj"]), ip(o["status"]), ip(o["iters"]), None, 0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    call = lambda b, sim, n=A: lib.srb12_rollout_device(s._h, n, ctypes.byref(b), ctypes.byref(sim), 1, st)
    # a wrong struct_size, with a live context
    sim = r._sim(); sim.struct_size += 8
    assert lib.srb12_sim_advance_device(s._h, A, ctypes.byref(sim), 0, st) == -1 and "srb12_sim.struct_size" in err()
    assert lib.srb12_sim_metrics_device(s._h, A, ctypes.byref(sim), 0, st) == -1 and "srb12_sim.struct_size" in err()
    assert call(batch(), sim) == -1 and "srb12_sim.struct_size" in err()
    assert call(batch(struct_size=8), r._sim()) == -1 and "srb12_batch.struct_size" in err()
    # a missing x
    sim = r._sim(); sim.x = None
    assert lib.srb12_sim_advance_device(s._h, A, ctypes.byref(sim), 1, st) == -1 and "srb12_sim.x" in err()
    # a sharded batch in the rollout
    assert call(batch(agent_offset=1), r._sim()) == -1 and "sharded" in err()
    assert call(batch(n_all=A + 1), r._sim()) == -1 and "sharded" in err()
    # N < 4
    s2 = srb12.Solver12(srb12.default_params(3, K_obs=1, K_nbr=0), 4)
    assert lib.srb12_sim_advance_device(s2._h, 4, ctypes.byref(r._sim()), 0, s2._stream(None)) == -1 and "N >= 4" in err()
    with pytest.raises(ValueError, match="N >= 4"):
        srb12.Rollout12(s2, dev(torch, goal[:4]))
    s2.close()
    # scenes: n_all not a multiple of scene_agents (the solves and the metrics), n_agents not whole scenes (the rollout)
    s.set_scenes(3, 1)
    try:
        b0 = sim12_oracle.cycle_inputs12(sim12_oracle.closed_loop12(run)["p"], state, goal, obstacles, 0, phase, gait)
        with pytest.raises(RuntimeError, match="is not a multiple of scene_agents"):
            s.solve(b0["x0"], b0["xref"], b0["foot"], b0["contact"], obstacles[:1], b0["nbr_state"])
        with pytest.raises(RuntimeError, match="is not a multiple of scene_agents"):
            s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, r.out)
        assert lib.srb12_sim_metrics_device(s._h, A, ctypes.byref(r._sim()), 0, st) == -1
        assert "is not a multiple of scene_agents" in err()
        with pytest.raises(ValueError, match="multiple of scene_agents"):
            r.run(1)
        assert call(batch(), r._sim()) == -1 and "rolls out whole scenes" in err() and "not a multiple of scene_agents" in err()
    finally:
        s.set_scenes(0, 0)
    with pytest.raises(ValueError, match="goal"):
        srb12.Rollout12(s, dev(torch, goal).float())
    with pytest.raises(ValueError, match="state"):
        r.reset(dev(torch, state)[:, :4])
    with pytest.raises(ValueError, match="gait"):
        srb12.Rollout12(s, dev(torch, goal), gait="pace")
    # after the refusals the same objects roll out as if nothing had happened
    r.reset(dev(torch, state))
    r.run(T)
    res = r.results()
    torch.cuda.synchronize()
    res = host(res)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
