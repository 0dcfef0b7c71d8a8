"""GPU tests of the disturbed plant of the SRB-12 rollout (csrc/srb12_plant.hip, srb12_sim_advance_plant_device,
srb12_rollout_plant_device, Rollout12(plant=Plant12(...))).

The kernels are compared with their numpy restatement (tests/plant12_oracle.py): the disturbance and everything that
does not pass through the roll's cos / sin bit for bit, Theta and omega of a rolled state within
sim12_oracle.TRIG_TOL times the roll's amplification (plant12_oracle.roll_amplification, derived there from the net
torque of the data).  The closed loop is checked per cycle from the device's own logs, so nothing drifts."""
import ctypes

import numpy as np
import pytest
from conftest import converged

import oracle
import plant12_oracle as p12
import sim12_oracle
import sim_oracle
import srbnmpc
import test_plant12
import test_rollout12_gpu as t12
from srbnmpc import srb12, workload

gpu = pytest.mark.gpu
TS = workload.TS
X_TOL, F_TOL, S_TOL = t12.X_TOL, t12.F_TOL, t12.S_TOL      # the SRB-12 parity tolerances (tests/test_srb12.py)
TRIG_TOL = sim12_oracle.TRIG_TOL
DYNTOL = 1e-8         # SRB12_POL_DYNTOL (csrc/srb_kernel_params.h): max_k |x_{k+1} - A_k x_k - B_k u_k - c_k| of an
#                       accepted polish, absolute
PLAIN, TRIG = [0, 1, 2, 6, 7, 8], [3, 4, 5, 9, 10, 11]      # p, v never see the roll's cos / sin; Theta, omega do
_need_gpu, solver, dev, host = t12._need_gpu, t12.solver, t12.dev, t12.host


def _dp(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._dp)


def _ip(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._ip)


def lin_points(state, xref, trace, at_state):
    """[A][4][3]: the positions the four steps of a roll linearise about."""
    if at_state:
        return np.stack([state[:, :3]] + [z[:, :3] for z in trace[:3]], 1)
    return np.concatenate([state[:, None, :3], xref[:, :3, :3]], 1)


def assert_state_equal(got, want, tol, where):
    """A state z + d against the restatement: p and v bit for bit, Theta and omega within tol (0: bit for bit)."""
    assert np.array_equal(got[:, PLAIN], want[:, PLAIN]), (where, "p, v")
    if tol == 0:
        assert np.array_equal(got[:, TRIG], want[:, TRIG]), (where, "Theta, omega")
        return 0.0
    err = np.abs(got[:, TRIG] - want[:, TRIG]).max()
    assert err <= tol, (where, err, tol)
    return err


# ================================================================================== 1. the kernels
def kernel_case12(A, N, seed):
    """Synthetic inputs (numpy only): states in the arena with yaws beyond +-pi, and a decision vector whose X at grid
    index 3 is a state of the same kind and whose forces are of walking size."""
    rng = np.random.default_rng(seed)

    def states():
        st = rng.normal(size=(A, 12)) * 0.05
        st[:, 0] = rng.uniform(0, 9, A); st[:, 1] = rng.uniform(-2, 2, A); st[:, 2] += 0.3
        st[:, 5] = rng.uniform(-4, 4, A); st[:, 6:8] = rng.uniform(-.3, .3, (A, 2))
        st[:, 9:12] = rng.uniform(-0.3, 0.3, (A, 3))
        return st
    state = states()
    goal = np.tile([10.0, 0.0], (A, 1))
    goal[3] = state[3, :2] - [3.0, 1.0]
    phase = rng.integers(0, 4, A).astype(np.int32)
    nv = 24 * N + 1
    x = rng.normal(size=(A, nv))
    x[:, 36:48] = states()
    U = x[:, 12 * N:24 * N].reshape(A, N, 4, 3)
    U[..., 2] = rng.uniform(20, 70, (A, N, 4))
    U[..., :2] = rng.uniform(-10, 10, (A, N, 4, 2))
    status = rng.integers(0, 5, (A, 2)).astype(np.int32); iters = rng.integers(0, 50, (A, 2)).astype(np.int32)
    return dict(state=state, goal=goal, phase=phase, x=x, status=status, iters=iters)


@gpu
@pytest.mark.parametrize("A,N,gait,what,with_phase,offset,n_all,at_state",
                         [(5, 4, "trot", "kick_v", False, 0, 5, 0), (300, 10, "trot", "all", True, 7, 320, 0),
                          (300, 4, "stand", "body", False, 0, 300, 0), (300, 4, "stand", "body", False, 0, 300, 1)])
def test_kernels_equal_the_restatement(A, N, gait, what, with_phase, offset, n_all, at_state):
    """srb12_sim_advance_plant_device at a first cycle (the caller's state, nothing of the plant: the nominal kernel)
    and at a later one.  The later cycle's roll reads the xref, foot and contact the first advance wrote, so the
    restatement is fed the device's own arrays.  A = 300 is a partial second block of the per-agent kernel; the shard of
    case two starts at global row 7 of 320; its six pushes hold two on one agent in the firing cycle (they add up in
    table order), one on a row outside the shard, one in another cycle, one at c_first (it does not fire) and one
    single."""
    torch = _need_gpu()
    s = solver(N, 1, 0)
    p, nv = s.params, s.params.nv
    k = kernel_case12(A, N, 2000 + A + N + at_state)
    state, goal, x, status, iters = (k[n] for n in ("state", "goal", "x", "status", "iters"))
    phase = k["phase"] if with_phase else None
    rng = np.random.default_rng(A + N)
    c0, c1, seed = 3, 6, 0x1234567890abcdef
    tab = dict(kick_v=rng.uniform(0.0, 0.1, n_all) if what in ("kick_v", "all") else None,
               kick_p=rng.uniform(0.0, 0.02, n_all) if what == "all" else None,
               kick_w=rng.uniform(0.0, 0.2, n_all) if what == "all" else None,
               mass=p.mass * rng.uniform(0.85, 1.15, n_all) if what in ("all", "body") else None,
               inertia=rng.uniform(0.8, 1.25, n_all) if what in ("all", "body") else None)
    pushes = None
    if what == "all":
        pushes = (np.array([c1, c1, c1, c1 + 1, c0, c1], np.int32),
                  np.array([offset + 4, 3, offset + 4, offset + 9, offset + 5, offset + 299], np.int32),
                  rng.uniform(-0.3, 0.3, (6, 6)))
    f8, i4 = torch.float64, torch.int32
    z = lambda *sh, dt=f8: torch.full(sh, -7, dtype=dt, device="cuda")
    t = dict(state=dev(torch, state), goal=dev(torch, goal), phase=None if phase is None else dev(torch, phase),
             x=dev(torch, x), status=dev(torch, status), iters=dev(torch, iters), x0=z(A, 12), xref=z(A, N, 12),
             foot=z(A, N, 4, 3), contact=z(A, N, 4, dt=i4), last_state=z(A, 4), com=z(A, 4), traj=z(c1 - c0 + 1, A, 12),
             status_log=z(c1 - c0, A, 2, dt=i4), iters_log=z(c1 - c0, A, 2, dt=i4), x_log=z(c1 - c0, A, nv),
             dist_log=z(c1 - c0, A, 12))
    tt = {n: None if v is None else dev(torch, v) for n, v in tab.items()}
    pt = [None] * 3 if pushes is None else [dev(torch, v) for v in pushes]
    sim = srb12.Sim12(_dp(t["state"]), _dp(t["goal"]), _ip(t["phase"]), 0.27, 0.3, 0.1, 0.05, srb12.GAITS[gait], c0,
                      _dp(t["x"]), _ip(t["status"]), _ip(t["iters"]), _dp(t["x0"]), _dp(t["xref"]), _dp(t["foot"]),
                      _ip(t["contact"]), _dp(t["last_state"]), _dp(t["com"]), _dp(t["traj"]), _ip(t["status_log"]),
                      _ip(t["iters_log"]), _dp(t["x_log"]), None, None, 0, n_all, offset, None, None, None, None, None,
                      None)
    plant = srb12.PlantStruct12(seed, _dp(tt["kick_v"]), _dp(tt["kick_p"]), _dp(tt["kick_w"]), _dp(tt["mass"]),
                                _dp(tt["inertia"]), at_state, 0 if pushes is None else 6, _ip(pt[0]), _ip(pt[1]),
                                _dp(pt[2]), _dp(t["dist_log"]))
    lib, st = srb12._lib(), s._stream(None)
    srbnmpc._check(lib.srb12_sim_advance_plant_device(s._h, A, ctypes.byref(sim), ctypes.byref(plant), c0, st))
    torch.cuda.synchronize()
    got0 = {n: (None if v is None else v.cpu().numpy()) for n, v in t.items()}
    w0 = sim12_oracle.advance12(N, TS, state, goal, 0.27, c0, phase, gait)
    t12.assert_advance_equal(got0, w0, c0)
    assert np.array_equal(got0["state"], state) and np.array_equal(got0["traj"][0], state)
    assert (got0["dist_log"] == -7).all() and (got0["x_log"] == -7).all() and (got0["traj"][1:] == -7).all()

    srbnmpc._check(lib.srb12_sim_advance_plant_device(s._h, A, ctypes.byref(sim), ctypes.byref(plant), c1, st))
    torch.cuda.synchronize()
    got = {n: (None if v is None else v.cpu().numpy()) for n, v in t.items()}
    rolls = what in ("all", "body")
    kw = dict(agent_offset=offset, seed=seed, pushes=pushes, at_state=bool(at_state), **tab)
    want, d = p12.plant_state12(p, c1, state, x, got0["xref"], got0["foot"], got0["contact"], **kw)
    r = c1 - c0 - 1
    np.testing.assert_array_equal(got["dist_log"][r], d)
    assert (got["dist_log"][:r] == -7).all() and (got["traj"][1:c1 - c0] == -7).all()
    tol = 0.0
    if rolls:
        m, Ibs = p12.body_tables(p, A, offset, tab["mass"], tab["inertia"])
        tr = p12.roll12(p, state, x, got0["xref"], got0["foot"], got0["contact"], m, Ibs, bool(at_state), trace=True)
        amp = p12.roll_amplification(p, x, got0["foot"], got0["contact"], lin_points(state, got0["xref"], tr, at_state),
                                     bool(at_state), tab["inertia"][offset:offset + A])
        tol = TRIG_TOL * amp
    err = assert_state_equal(got["state"], want, tol, (what, at_state))
    print(f"case {(A, N, gait, what, at_state)}: max |device - numpy| of Theta, omega {err:.3e} (tolerance {tol:.3e})")
    # everything the advance derives from the state, from the device's own state
    w = sim12_oracle.advance12(N, TS, got["state"], goal, 0.27, c1, phase, gait)
    t12.assert_advance_equal(got, w, c1)
    assert np.array_equal(got["traj"][c1 - c0], got["state"])
    assert np.array_equal(got["status_log"][r], status) and np.array_equal(got["iters_log"][r], iters)
    assert np.array_equal(got["x_log"][r], x)
    if what == "kick_v":
        assert (d[:, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]] == 0).all() and (d[:, 6:8] != 0).all()
        assert (np.abs(d[:, 6:8]) < tab["kick_v"][:, None]).all()
        rest = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]
        np.testing.assert_array_equal(got["state"][:, rest], x[:, 36:48][:, rest])
    if what == "body":
        assert (d == 0).all() and (got["state"][:, 6:12] != x[:, 42:48]).all()      # the roll, not the prediction
        other = p12.plant_state12(p, c1, state, x, got0["xref"], got0["foot"], got0["contact"],
                                  **dict(kw, at_state=not at_state))[0]
        # the other linearisation point is another roll
        assert np.abs(got["state"][:, 9:12] - other[:, 9:12]).max() > 1e3 * max(tol, TRIG_TOL)
    if what == "all":
        u = p12.plant_oracle.kicks(seed, c1, offset + np.arange(A))
        kv = tab["kick_v"]
        assert d[4, 6] == (0.0 + kv[offset + 4] * u[4, 0] + pushes[2][0, 0]) + pushes[2][2, 0]          # table order
        assert d[299, 6] == 0.0 + kv[offset + 299] * u[299, 0] + pushes[2][5, 0]
        assert d[9, 6] == 0.0 + kv[offset + 9] * u[9, 0] and d[5, 6] == 0.0 + kv[offset + 5] * u[5, 0]   # not due, at c_first
        uw = p12.angular_kicks(seed, c1, offset + np.arange(A))
        assert d[4, 11] == (0.0 + tab["kick_w"][offset + 4] * uw[4, 2] + pushes[2][0, 5]) + pushes[2][2, 5]
        assert (d[:, 2:6] == 0).all()


# ================================================================================== the closed loop
def make_rollout(torch, run, plans=False, plant=None, **kw):
    A, N, gait, seed, T, Ko, Kn = run
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                        obstacles=dev(torch, obstacles), plans=plans, plant=plant, **kw)
    r.reset(dev(torch, state))
    return r


def drive(r, T, plant="agents"):
    """T cycles of the Rollout12 r (after reset) by the C driver, called directly: srb12_rollout_agents_device, or
    srb12_rollout_plant_device with `plant` (None, or a srb12.PlantStruct12)."""
    s, o = r.solver, r.out
    r._reserve(T)
    b = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], r.A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
    pl = ctypes.byref(srb12.Plans12(None, _dp(o["plan"]), 0, _dp(r.plan_table))) if r.plans else None
    lib = srb12._lib()
    if plant == "agents":
        rc = lib.srb12_rollout_agents_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), pl, None, None, None, T,
                                             s._stream(None))
    else:
        rc = lib.srb12_rollout_plant_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), pl, None, None, None,
                                            None if plant is None else ctypes.byref(plant), T, s._stream(None))
    srbnmpc._check(rc)
    r.c, r.flushed = T, True
    return host(r.results())


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_nothing_set_is_the_nominal_path_bitwise(plans):
    """plant NULL and a struct with nothing set (and a dist_log, which then stays unwritten) give the bits of
    srb12_rollout_agents_device through the driver, and of srb12_sim_advance_device through the advance entry point
    (step() of a Rollout12 made to pass such a struct): traj, the logs and every metric, 8 agents, 5 cycles."""
    torch = _need_gpu()
    run, T = sim12_oracle.RUNS12[2], 5
    A = run[0]
    dist = torch.full((T, A, 12), -7.0, dtype=torch.float64, device="cuda")
    empty = srb12.PlantStruct12(99, None, None, None, None, None, 0, 0, None, None, None, _dp(dist))
    res = [drive(make_rollout(torch, run, plans), T, kw) for kw in ("agents", None, empty)]
    assert (dist == -7).all()
    # the Python layer with a Plant12 that sets nothing: the nominal object
    r = make_rollout(torch, run, plans, plant=srb12.Plant12(seed=5))
    assert r.plant is None
    # ... and made to pass the empty struct through both plant entry points all the same
    for mode in ("run", "step"):
        r = make_rollout(torch, run, plans)
        r.plant = srb12.Plant12(seed=5)
        r._reserve(T)
        r.dist_log.fill_(-7.0)
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        out = host(r.results())
        assert (out.pop("disturbance") == -7).all()
        res.append(out)
    assert "disturbance" not in res[0]
    for other in res[1:]:
        assert sorted(other) == sorted(res[0])
        for k, v in res[0].items():
            assert np.array_equal(other[k], v), k
    assert res[0]["traj"].shape == (T + 1, A, 12) and not np.array_equal(res[0]["traj"][T], res[0]["traj"][0])


def dynamics_bound(p, res, R, gait, steps=4):
    """(a, S): the growth |A_k|_inf <= a = 1 + Ts sqrt2 and the largest sum of term magnitudes of a step over the logged
    agent-cycles (test_plant12.roll_bound's S)."""
    T, A = res["status"].shape[:2]
    N = p.N
    S = 0.0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], R["goal"], R["obstacles"], c, R["phase"], gait)
        for a in range(A):
            Ak, Bk, ck = oracle.dynamics12(p, b["x0"][a], b["xref"][a], b["foot"][a], b["contact"][a])
            X = np.concatenate([b["x0"][a][None], res["x"][c][a, :12 * N].reshape(N, 12)])
            U = res["x"][c][a, 12 * N:24 * N].reshape(N, 12)
            for k in range(steps):
                S = max(S, (np.abs(Ak[k]) @ np.abs(X[k]) + np.abs(Bk[k]) @ np.abs(U[k]) + np.abs(ck[k])).max())
    return 1.0 + TS * np.sqrt(2.0), S


@gpu
def test_the_model_is_its_own_plant():
    """mass = the model's, inertia = 1, at_state 0, no kicks: the plant's roll from x0 under U_0 .. U_3 ends at X at grid
    index 3.  An OPTIMAL solve is polished and its dynamics rows hold to DYNTOL (absolute, every k), so the roll agrees
    within the residuals carried through the later steps, DYNTOL (1 + a + a^2 + a^3) with |A_k|_inf <= a = 1 + Ts sqrt2,
    plus the roll's own rounding (test_plant12: 104 u S per step, carried the same way).  The run is one whose
    oracle-only closed loop is OPTIMAL in every agent-cycle (chosen on the CPU), and none is left out on the device.
    With at_state 1 from a start at zero omega the first step still coincides with the model's (both linearise about
    the start state); the later ones do not: the end state differs from X_3 and equals the restatement."""
    torch = _need_gpu()
    run = sim12_oracle.RUNS12[3]
    A, N, gait, seed, T, Ko, Kn = run
    R = sim12_oracle.closed_loop12(run)
    assert (R["status"][:, :, 1] == 0).all() and converged(R["status"].reshape(-1, 2)).all()     # the oracle: all OPTIMAL
    p = R["p"]
    s = solver(N, Ko, Kn)
    ones = dev(torch, np.ones(A))
    r = make_rollout(torch, run, plant=srb12.Plant12(mass=dev(torch, np.full(A, s.params.mass)), inertia=ones))
    r.run(T)
    res = host(r.results())
    assert converged(res["status"].reshape(-1, 2)).all() and (res["disturbance"] == 0).all()      # none left out
    a, S = dynamics_bound(p, res, R, gait)
    G = 1 + a + a ** 2 + a ** 3
    bound = DYNTOL * G + test_plant12.ROLL_K * test_plant12.U_ROUND * S * G
    err = np.abs(res["traj"][1:] - res["x"][:, :, 36:48]).max()
    print(f"a {a:.6f} S {S:.3f} bound {bound:.3e}; {T * A} agent-cycles, all OPTIMAL: max |roll - X3| {err:.3e}")
    assert err <= bound, (err, bound)
    assert (res["traj"][1:] != res["x"][:, :, 36:48]).any()                  # ... and it is the roll that was stored

    # at_state 1, zero omega at the start; two cycles (the first is the nominal rollout's problem: all OPTIMAL)
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    state = state.copy()
    state[:, 9:12] = 0.0
    r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, obstacles),
                        plant=srb12.Plant12(at_state=True))
    r.reset(dev(torch, state))
    T1 = 2
    r.run(T1)
    res1 = host(r.results())
    assert np.array_equal(res1["traj"][0], state) and converged(res1["status"][0]).all()
    m, Ibs = p12.body_tables(p, A)
    worst = first = 0.0
    round1 = test_plant12.ROLL_K * test_plant12.U_ROUND * S
    for c in range(T1):
        b = sim12_oracle.cycle_inputs12(p, res1["traj"][c], goal, obstacles, c, phase, gait)
        tr = p12.roll12(p, res1["traj"][c], res1["x"][c], b["xref"], b["foot"], b["contact"], m, Ibs, True, trace=True)
        ok = converged(res1["status"][c])
        pts = lin_points(res1["traj"][c], b["xref"], tr, 1)
        if ok.any():
            # the first step against X at grid index 0: the polish's residual, the step's rounding, the rebuilt footholds
            amp0 = p12.roll_amplification(p, res1["x"][c], b["foot"], b["contact"], pts, False, rebuilt=True, steps=1)
            e0 = np.abs(tr[0][ok] - res1["x"][c][ok, 0:12]).max()
            assert e0 <= DYNTOL + round1 + TRIG_TOL * amp0, (c, e0)
            first = max(first, e0)
        amp = p12.roll_amplification(p, res1["x"][c], b["foot"], b["contact"], pts, True, rebuilt=True)
        worst = max(worst, assert_state_equal(res1["traj"][c + 1], tr[3], TRIG_TOL * amp, ("at_state", c)))
    off = np.abs(res1["traj"][1] - res1["x"][0][:, 36:48]).max()
    print(f"at_state 1: first step within {first:.3e} of X_0 (bound {DYNTOL + round1:.3e} + the footholds'); end state "
          f"{off:.3e} from X_3 after one cycle; |device - numpy| {worst:.3e}")
    assert off > 100 * bound


def spread_team12(A, N, gait, seed):
    """workload.make_batch12's states, obstacles and phases with the starts moved onto a 2.2 m grid (yaws turned to
    the goal's new bearing, the drawn offset kept), every goal at GOAL: over six cycles (0.3 m of travel) no pair
    comes within sqrt(eps_nbr) = 1.48 m, so the inter-agent rows -- which the device predicts by the neighbours'
    shifted plans and oracle.solve_batch12 by constant velocity -- are inactive and the two problems share their
    optimum."""
    b = workload.make_batch12(A, N, gait, seed=seed)
    state = np.array(b["x0"], dtype=np.float64)
    goal = np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1))
    old = np.arctan2(goal[:, 1] - state[:, 1], goal[:, 0] - state[:, 0])
    cols = (A + 1) // 2
    state[:, 0] = 0.4 + 2.2 * (np.arange(A) % cols)
    state[:, 1] = np.where(np.arange(A) < cols, -1.2, 1.2)
    state[:, 5] += np.arctan2(goal[:, 1] - state[:, 1], goal[:, 0] - state[:, 0]) - old
    phase = np.random.default_rng(seed).integers(0, 4, A).astype(np.int32)
    return state, goal, np.array(b["obstacles"], dtype=np.float64), phase


LOOP = (8, 4, "trot", 6, 6, 1, 2)      # (A, N, gait, seed, T, K_obs, K_nbr) of the disturbed closed loop
_loop = {}


def loop_tables(A):
    kv, kp, kw, mass, inertia = workload.plant_tables12(A, 3)
    push = (np.array([3], np.int32), np.array([5], np.int32), np.array([[0.15, -0.1, 0.05, 0.2, -0.1, 0.3]]))
    return dict(kick_v=kv, kick_p=kp, kick_w=kw, mass=mass, inertia=inertia, pushes=push)


def disturbed12(mode="run", agent_rad=False):
    """The disturbed rollout of LOOP on the device (plans on, drawn tables, one push, seed 11) with log_x, once per
    (mode, agent_rad): host copies of results()."""
    if (mode, agent_rad) not in _loop:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = LOOP
        state, goal, obstacles, phase = spread_team12(A, N, gait, seed)
        tab = loop_tables(A)
        plant = srb12.Plant12(11, *(dev(torch, tab[n]) for n in ("kick_v", "kick_p", "kick_w", "mass", "inertia")),
                              False, tuple(dev(torch, v) for v in tab["pushes"]))
        kw = dict(agent_rad=dev(torch, np.full(A, 0.7))) if agent_rad else {}
        r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                            obstacles=dev(torch, obstacles), plans=True, plant=plant, **kw)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        _loop[(mode, agent_rad)] = host(r.results())
    return _loop[(mode, agent_rad)]


@gpu
def test_disturbed_closed_loop_every_cycle_from_the_logs():
    A, N, gait, seed, T, Ko, Kn = LOOP
    state, goal, obstacles, phase = spread_team12(A, N, gait, seed)
    tab = loop_tables(A)
    res = disturbed12()
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    assert res["cycles"] == T and res["disturbance"].shape == (T, A, 12) and np.array_equal(res["traj"][0], state)
    ex = eu = es = worst = 0.0
    compared = 0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], goal, obstacles, c, phase, gait)
        o = sim12_oracle.solve12(p, b)
        opt = converged(o["status"])
        assert np.array_equal(res["status"][c][opt], o["status"][opt]), (c, res["status"][c].tolist(), o["status"].tolist())
        compared += int(opt.sum())
        g, w = res["x"][c][opt], o["x"][opt]
        if opt.any():
            ex = max(ex, np.abs(g[:, :12 * N] - w[:, :12 * N]).max())
            eu = max(eu, np.abs(g[:, 12 * N:24 * N] - w[:, 12 * N:24 * N]).max())
            es = max(es, np.abs(g[:, -1] - w[:, -1]).max())
        want, d = p12.plant_state12(p, c + 1, res["traj"][c], res["x"][c], b["xref"], b["foot"], b["contact"], seed=11, **tab)
        np.testing.assert_array_equal(res["disturbance"][c], d, err_msg=f"cycle {c}")
        m, Ibs = p12.body_tables(p, A, 0, tab["mass"], tab["inertia"])
        tr = p12.roll12(p, res["traj"][c], res["x"][c], b["xref"], b["foot"], b["contact"], m, Ibs, False, trace=True)
        amp = p12.roll_amplification(p, res["x"][c], b["foot"], b["contact"], lin_points(res["traj"][c], b["xref"], tr, 0),
                                     False, tab["inertia"], rebuilt=True)
        worst = max(worst, assert_state_equal(res["traj"][c + 1], want, TRIG_TOL * amp, c))
    assert np.array_equal(res["state"], res["traj"][T])
    d = res["disturbance"]
    off = np.abs(res["traj"][1:] - res["x"][:, :, 36:48]).max()
    print(f"{LOOP}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; next state "
          f"|device - numpy| {worst:.3e}; largest departure from the prediction {off:.4f}; min_d_agent "
          f"{res['min_d_agent'].min():.4f} min_d_obs {res['min_d_obs'].min():.4f}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    assert d[2, 5, 6] != 0 and (d[:, :, 2:6] == 0).all() and (d[:, :, [0, 1, 6, 7, 9, 10, 11]] != 0).all()
    assert np.abs(d[:, :, 0:2]).max() < 0.01 and np.abs(d[:, :, 9:12]).max() <= 0.1 + 0.3 and off > 0.01
    assert res["min_d_agent"].min() > 1.7                                      # the inter-agent rows stay inactive


@gpu
def test_c_driver_equals_python_steps_bitwise_with_the_plant_plans_and_agent_sizes():
    a, b = disturbed12("run", True), disturbed12("step", True)
    assert sorted(a) == sorted(b) and "disturbance" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["disturbance"], disturbed12("run", False)["disturbance"])   # the draws do not depend on it


@gpu
def test_replicas_of_one_scene_draw_by_their_global_rows_and_the_lip_draws():
    """workload.replicate_scenes of one 4-agent make_scenes12 scene x 8 under set_scenes: without kicks every replica is
    the same rollout; with kick_v 0.05 and kick_p 0.005 every replica has its own draws, the restatement's at its global
    rows; the same seed gives the same bits, another seed another disturbance; and the planar columns of the log are
    the LIP Rollout's disturbance for the same seed, bounds and rows, bit for bit."""
    torch = _need_gpu()
    team, n_obs, copies, N, T = 4, 5, 8, 4, 4
    sc = workload.replicate_scenes(workload.make_scenes12(1, team, N, "trot", seed=2, n_obs=n_obs), copies)
    A = team * copies
    s = srb12.Solver12(srb12.default_params(N, K_obs=1, K_nbr=2), A)
    s.set_scenes(team, n_obs)

    def roll(kick, seed):
        plant = srb12.Plant12(seed, dev(torch, np.full(A, kick)), dev(torch, np.full(A, kick / 10)))
        r = srb12.Rollout12(s, dev(torch, sc["goal"]), phase=dev(torch, sc["phase"]), log_x=True,
                            obstacles=dev(torch, sc["obstacles"]), plant=plant)
        r.reset(dev(torch, sc["x0"]))
        r.run(T)
        out = host(r.results())
        out["scenes"] = host(r.scene_results())
        return out
    calm = roll(0.0, 5)
    per = calm["traj"].reshape(T + 1, copies, team, 12)
    assert (calm["disturbance"] == 0).all() and (per == per[:, :1]).all()
    a, again, other = roll(0.05, 5), roll(0.05, 5), roll(0.05, 6)
    for k in a:
        if k != "scenes":
            assert np.array_equal(a[k], again[k]), k
    assert not np.array_equal(a["disturbance"], other["disturbance"])
    d = a["disturbance"].reshape(T, copies, team, 12)
    for i in range(copies):
        for j in range(i):
            assert (d[:, i] != d[:, j])[..., [0, 1, 6, 7]].all(), (i, j)
    for c in range(T):
        st, dd = p12.plant_state12(s.params, c + 1, a["traj"][c], a["x"][c], seed=5, kick_v=np.full(A, 0.05),
                                   kick_p=np.full(A, 0.005))
        np.testing.assert_array_equal(a["disturbance"][c], dd)
        np.testing.assert_array_equal(a["traj"][c + 1], st)
    assert a["scenes"]["n_scenes"] == copies and a["scenes"]["min_d_agent"].shape == (copies,)
    s.close()
    # the LIP rollout of as many agents with the same seed and bounds: the same planar kicks
    C = 2
    lstate, lgoal, lobs = sim_oracle.team(A, N, C, 9)
    ls = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=1, K_nbr=2), A)
    lr = srbnmpc.Rollout(ls, dev(torch, lgoal), obstacles=dev(torch, lobs), plant_seed=5, kick_v=dev(torch, np.full(A, 0.05)),
                         kick_p=dev(torch, np.full(A, 0.005)))
    lr.reset(dev(torch, lstate))
    lr.run(T)
    ld = host(lr.results())["disturbance"]                                 # (dpx, dvx, dpy, dvy)
    ls.close()
    assert np.array_equal(a["disturbance"][:, :, [0, 6, 1, 7]], ld)


@gpu
def test_refusals_by_name_on_a_live_context_and_it_survives():
    torch = _need_gpu()
    run = sim12_oracle.RUNS12[2]
    A, N, gait, seed, T, Ko, Kn = run
    r = make_rollout(torch, run, plans=True)
    s = r.solver
    r._reserve(2)
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    o = r.out
    b = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
    keep, cases = test_plant12.refusal_cases()
    for plant, word, missing in cases:
        sim = r._sim()
        if missing:
            if missing == "x":
                continue                                      # srb12_sim.x missing is the advance's own refusal, first
            setattr(sim, missing, None)
        else:
            assert test_plant12.call_refused(lib, s._h, "rollout", plant, sim, b, A) == -1 and word in err(), word
        assert test_plant12.call_refused(lib, s._h, "advance", plant, sim, None, A) == -1 and word in err(), word
    tab = dev(torch, np.full(A + 1, 0.01))
    on = srb12.PlantStruct12(1, _dp(tab), None, None, None, None, 0, 0, None, None, None, None)
    sim = r._sim(); sim.agent_offset = 2; sim.n_all = A + 1       # rows 2 .. A + 1 of an (A + 1)-row table
    assert lib.srb12_sim_advance_plant_device(s._h, A, ctypes.byref(sim), ctypes.byref(on), 1, s._stream(None)) == -1
    assert "srb12_plant: agent_offset + n_agents exceeds n_all" in err()
    b.agent_offset = 1                                            # a shard cannot roll out alone, plant or not
    assert test_plant12.call_refused(lib, s._h, "rollout", on, r._sim(), b, A) == -1 and "sharded" in err()
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    for plant, word in ((srb12.Plant12(kick_v=dev(torch, np.full(A + 1, 0.1))), "kick_v must have one row per agent"),
                        (srb12.Plant12(mass=torch.ones(A, dtype=torch.float64)), "mass must be on"),
                        (srb12.Plant12(pushes=(dev(torch, np.array([1], np.int32)), dev(torch, np.array([A], np.int32)),
                                               dev(torch, np.zeros((1, 6))))), "pushes: agent"),
                        (dict(kick_v=None), "plant must be a srb12.Plant12")):
        with pytest.raises(ValueError, match=word):
            srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, obstacles), plant=plant)
    with pytest.raises(ValueError, match="Plant12: inertia must be > 0"):
        srb12.Plant12(inertia=dev(torch, np.zeros(A)))
    with pytest.raises(ValueError, match="Rollout12: kick_v is not available"):
        srb12.Rollout12(s, dev(torch, goal), kick_v=dev(torch, np.full(A, 0.1)))
    # after the refusals a plain rollout on the same context gives the bits it always gave
    r = make_rollout(torch, run)
    r.run(T)
    res = host(r.results())
    want = t12.rollout12(run)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
