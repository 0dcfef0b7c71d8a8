"""GPU tests of the degraded neighbour link of the SRB-12 mode (srb12_link_update_device,
srb12_solve_batch_link_device, srb12_rollout_link_device; Solver12.solve_device(own_plan=), Rollout12(link=...)).

The selection kernels with an own plan are compared exactly with tests/link12_oracle.select_own; the link update through
an SRB-12 context bit for bit with tests/link_oracle.py; the closed loop per cycle from the device's own logs: what is
seen is the restatement of the logged truth, bitwise, every converged solve agrees with the oracle fed the PERCEIVED
tables at the SRB-12 tolerances, and the metrics are sim_oracle's on the TRUE states."""
import ctypes

import numpy as np
import pytest

import link12_oracle as l12
import link_oracle
import oracle
import plan12_oracle as po
import sim12_oracle
import sim_oracle
import srbnmpc
import test_link_gpu as tlg
import test_rollout12_gpu as t12
from srbnmpc import srb12, workload

gpu = pytest.mark.gpu
TS = workload.TS
X_TOL, F_TOL, S_TOL = t12.X_TOL, t12.F_TOL, t12.S_TOL       # tests/test_srb12.py
_need_gpu, solver, dev, host = t12._need_gpu, t12.solver, t12.dev, t12.host
_dp, _ip, guarded = tlg._dp, tlg._ip, tlg.guarded
FILL, GUARD = tlg.FILL, tlg.GUARD


# ================================================================================== 1. the selection kernels
_sel_solvers = {}


def sel_solver(N, Kn):
    """A Solver12 for the selection tests: one static column, K_nbr neighbour columns, two iterations a stage (the
    test reads sel alone; the selection precedes the solve and does not depend on it)."""
    if (N, Kn) not in _sel_solvers:
        _sel_solvers[(N, Kn)] = srb12.Solver12(srb12.default_params(N, K_obs=1, K_nbr=Kn, qp_maxit=2, nlp_maxit=2), 320)
    return _sel_solvers[(N, Kn)]


def crossing(pos, N, seed):
    """Crossing plans around pos [n][2] (test_nbr_plan12_gpu.crossing12): fast velocities and a curvature term."""
    rng = np.random.default_rng(seed)
    n = pos.shape[0]
    vel, acc = rng.normal(0, 12.0, (n, 2)), rng.normal(0, 40.0, (n, 2))
    t = TS * np.arange(1, N + 1)
    return np.ascontiguousarray(pos[:, None] + vel[:, None] * t[None, :, None] + 0.5 * acc[:, None] * (t * t)[None, :, None])


# (n_all, N, K_nbr, scene_agents, a NaN row); scene_agents 0: srb_knn_plan_kernel, else srb_knn_plan_scene_kernel
SEL_CASES = [(2, 10, 2, 0, False), (3, 10, 2, 0, True), (5, 4, 2, 0, False), (300, 10, 2, 0, False), (300, 10, 8, 0, False),
             (300, 10, 16, 0, False), (2, 10, 2, 2, False), (3, 10, 2, 3, True), (5, 4, 2, 5, False), (300, 10, 2, 30, False),
             (300, 10, 8, 30, False), (300, 10, 16, 30, False), (12, 10, 2, 4, False)]


@gpu
@pytest.mark.parametrize("n_all,N,Kn,scene,nan_row", SEL_CASES)
def test_selection_with_an_own_plan_equals_the_restatement(n_all, N, Kn, scene, nan_row):
    """sel of a solve whose table is what the agents perceive (positions off by centimetres, other plans) and whose
    own plans are the truth, against link12_oracle.select_own, exactly; without an own plan the kernel's old loads:
    the plain restatement on the perceived table, which is what the parent computes.  n_all = 2 with K_nbr = 2 is one
    real neighbour: the C ABI clamps the neighbour columns to the n_all - 1 rows that exist, so the -1 column is
    reached with a third row that cannot be selected (NaN in its perceived position).  300 rows are five scans a
    thread (two waves) and, with K_nbr 2, 8 and 16, the three insertion depths; (12, 4) is scenes of 4 agents x 3, (300,
    30) scenes wide enough for all three depths.  The truth row of every agent is another draw than its perceived row,
    and the test asserts that this changes some agent's columns.  A guard behind sel stays untouched."""
    torch = _need_gpu()
    s = sel_solver(N, Kn)
    b = workload.make_batch12(n_all, N, "trot", seed=400 + n_all + Kn)
    rng = np.random.default_rng(500 + n_all + Kn + scene)
    n_scenes = n_all // scene if scene else 1
    so = 2
    obstacles = rng.uniform(-2, 12, (n_scenes * so, 2))
    pos = b["nbr_state"][:, :2]
    seen = np.array(b["nbr_state"])
    seen[:, :2] += rng.uniform(-0.03, 0.03, (n_all, 2))
    if nan_row:
        seen[2, 0] = np.nan
    seen_plan, own = crossing(pos, N, 600 + n_all), crossing(pos, N, 700 + n_all)
    s.set_scenes(scene, so if scene else 0)
    try:
        Ko, kn = srb12.n_selected(s.params, obstacles.shape[0], n_all, s.scenes)
        assert Ko == 1 and kn == min(Kn, (scene or n_all) - 1)
        t = dict(x0=dev(torch, b["x0"]), xref=dev(torch, b["xref"]), foot=dev(torch, b["foot"]),
                 contact=dev(torch, b["contact"], torch.int32))
        d_ob, d_seen, d_plan, d_own = (dev(torch, a) for a in (obstacles, seen, seen_plan, own))
        got = {}
        for name, op in (("null", None), ("own", d_own)):
            flat, sel = guarded(torch, (n_all, Ko + kn), torch.int32)
            o = t12_out(torch, s, n_all)
            o["sel"] = sel
            s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], d_ob, d_seen, o, nbr_plan=d_plan,
                           plan_selection=True, own_plan=op)
            torch.cuda.synchronize()
            assert (flat[-GUARD:] == FILL).all(), name
            got[name] = sel.cpu().numpy()
            kernel = s.last_kernel()
        # the snapshot selection of the same call: the static columns, which no plan touches
        flat, sel = guarded(torch, (n_all, Ko + kn), torch.int32)
        o = t12_out(torch, s, n_all)
        o["sel"] = sel
        s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], d_ob, d_seen, o, nbr_plan=d_plan)
        torch.cuda.synchronize()
        snap = sel.cpu().numpy()
        assert s.last_kernel() == kernel                       # the solve kernel does not depend on the own plan
    finally:
        s.set_scenes(0, 0)
    x0 = l12.lip_rows(b["x0"])
    want_null = l12.select_own(x0, seen, seen_plan, None, kn, scene_agents=scene)
    want_own = l12.select_own(x0, seen, seen_plan, own, kn, scene_agents=scene)
    assert np.array_equal(got["null"][:, Ko:], want_null), np.where((got["null"][:, Ko:] != want_null).any(1))[0]
    assert np.array_equal(got["own"][:, Ko:], want_own), np.where((got["own"][:, Ko:] != want_own).any(1))[0]
    assert np.array_equal(got["null"][:, :Ko], snap[:, :Ko]) and np.array_equal(got["own"][:, :Ko], snap[:, :Ko])
    differ = int((got["own"] != got["null"]).any(1).sum())
    print(f"{n_all} rows, N {N}, K_nbr {Kn} -> {kn}, scenes of {scene}: the own plan changes the columns of {differ} agents")
    if kn < (scene or n_all) - 1 - int(nan_row):               # (else every row that can be selected is: n_all = 2 has
        assert differ >= 1                                      # one candidate, whatever the agent's own plan)
    if nan_row:
        assert (got["own"][:2, Ko:] == [[1, -1], [0, -1]]).all() and (got["null"][:2, Ko:] == [[1, -1], [0, -1]]).all()
    if scene:                                                  # global rows of the agent's scene alone
        sc = np.arange(n_all)[:, None] // scene
        for v in (got["own"][:, Ko:], got["null"][:, Ko:]):
            assert ((v // scene == sc) | (v < 0)).all()


def t12_out(torch, s, A):
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    nv = s.params.nv
    return dict(x=torch.zeros((A, nv), **f8), obj=torch.zeros(A, **f8), status=torch.zeros((A, 2), **i4),
                iters=torch.zeros((A, 2), **i4))


@gpu
def test_the_link_entry_point_without_an_own_plan_is_the_agents_entry_point_bitwise():
    """srb12_solve_batch_link_device(own_plan = NULL) called directly against Solver12.solve_device's old path
    (srb12_solve_batch_plans_device): every output and the kernel name, plan selection on and off."""
    torch = _need_gpu()
    N, Ko, Kn, A = 4, 1, 2, 8
    s = solver(N, Ko, Kn)
    b = workload.make_batch12(A, N, "trot", seed=45)
    table = dev(torch, crossing(b["nbr_state"][:, :2], N, 3))
    t = {k: dev(torch, b[k]) for k in ("x0", "xref", "foot", "obstacles", "nbr_state")}
    t["contact"] = dev(torch, b["contact"], torch.int32)
    lib = srb12._lib()
    for psel in (0, 1):
        outs, names = [], []
        for direct in (False, True):
            o = t12_out(torch, s, A)
            o["sel"] = torch.full((A, Ko + Kn), FILL, dtype=torch.int32, device="cuda")
            o["plan"] = torch.full((A, N, 2), float(FILL), dtype=torch.float64, device="cuda")
            if direct:
                bat = srb12.Batch12(_dp(t["x0"]), _dp(t["xref"]), _dp(t["foot"]), _ip(t["contact"]), _dp(t["obstacles"]),
                                    _dp(t["nbr_state"]), t["obstacles"].shape[0], A, 0, None, _dp(o["x"]), _dp(o["obj"]),
                                    _ip(o["status"]), _ip(o["iters"]), _ip(o["sel"]), 0)
                pl = srb12.Plans12(_dp(table), _dp(o["plan"]), psel, None)
                srbnmpc._check(lib.srb12_solve_batch_link_device(s._h, A, ctypes.byref(bat), ctypes.byref(pl), None, None,
                                                                 None, None, s._stream(None)))
            else:
                s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o,
                               nbr_plan=table, plan_selection=bool(psel))
            torch.cuda.synchronize()
            outs.append(host(o)); names.append(s.last_kernel())
        assert names[0] == names[1] and names[0].startswith("srb12_kernel_")
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[1][k]), (psel, k)


# ================================================================================== 2. the link update, bitwise
@gpu
def test_link_update_through_an_srb12_context_equals_the_restatement_bitwise():
    """srb12_link_update_device over cycles 0 .. 6 with random truth tables per cycle, no solve: every table, max_delay 3,
    extrapolate, N = 4 -- so from age 1 on all of a seen plan lies past the horizon (4 age >= N) -- and 300 rows (a
    partial last block).  Seen tables, age and every state buffer against link_oracle after every cycle; every buffer
    starts at a sentinel with a guard behind it."""
    torch = _need_gpu()
    n, N, D, T, c0 = 300, 4, 3, 7, 0
    rng = np.random.default_rng(1204)
    delay = rng.integers(0, D + 1, n).astype(np.int32)
    delay[:6] = [0, D, D + 5, -2, 1, 2]                        # two entries outside the ring: clamped
    drop = rng.uniform(0, 0.5, n)
    drop[:7], drop[7] = 0.0, 1.0
    tab = link_oracle.tables(0xfedcba9876543210, delay, drop, rng.uniform(0, 0.03, n), rng.uniform(0, 0.05, n), D, 1)
    s = solver(N, 1, 2)
    assert s.params.Ts == tab["Ts"]
    st = np.stack([rng.uniform(0, 9, (T, n)), rng.uniform(-2, 2, (T, n)), rng.uniform(-.3, .3, (T, n)),
                   rng.uniform(-.3, .3, (T, n))], -1)
    pl = rng.uniform(-3, 12, (T, n, N, 2))
    want = link_oracle.run(c0, st, pl, tab, N, FILL)
    lib, stream = srb12._lib(), s._stream(None)
    d_st, d_pl = dev(torch, st), dev(torch, pl)
    flat, buf = tlg.link_buffers(torch, n, N, D, T + 1)
    keep = {}
    link = tlg.link_struct(torch, tab, buf, keep)
    for i in range(T):
        srbnmpc._check(lib.srb12_link_update_device(s._h, n, ctypes.byref(link), _dp(d_st[i]), _dp(d_pl[i]), c0 + i, c0,
                                                    stream))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in buf.items()}
        seen, seen_plan, age, state = want[i]
        msg = f"cycle {c0 + i}"
        np.testing.assert_array_equal(got["seen_state"], seen, err_msg=msg)
        np.testing.assert_array_equal(got["age_log"][i], age, err_msg=msg)
        assert (got["age_log"][i + 1:] == FILL).all(), msg
        if seen_plan is None:
            assert i == 0 and (got["seen_plan"] == FILL).all(), msg
        else:
            np.testing.assert_array_equal(got["seen_plan"], seen_plan, err_msg=msg)
        for k, v in state.items():
            np.testing.assert_array_equal(got[k], v, err_msg=f"{msg}: {k}")
    for k, v in flat.items():
        assert (v[-GUARD:] == FILL).all(), k
    ages = np.array([w[2] for w in want])
    assert ages.max() > 3 and (ages[:, 7] == np.arange(T)).all() and (ages[4:, 2] == 3).all() and (ages[:, 3] == 0).all()
    # an aged row's whole seen plan is the line past its held horizon
    i = T - 1
    g = int(np.nonzero((ages[i] >= 1) & (want[i][3]["held_cycle"] > c0))[0][0])
    held = want[i][3]["held_plan"][g]
    e = held[N - 1] - held[N - 2]
    np.testing.assert_array_equal(want[i][1][g], np.array([held[N - 1] + float(k + 4 * ages[i, g] - N + 1) * e for k in range(N)]))


# ================================================================================== 3. the closed loop
def link_model(torch, A, tab):
    return srbnmpc.LinkModel(seed=tab["seed"], delay=dev(torch, tab["delay"]), drop=dev(torch, tab["drop"]),
                             noise_p=dev(torch, tab["noise_p"]), extrapolate=bool(tab["extrapolate"]))


@gpu
@pytest.mark.parametrize("extrapolate", [False, True])
def test_closed_loop_every_cycle_from_the_logs(extrapolate):
    """8 agents walking at each other (link12_oracle.head_on_team12), N = 4, trot, plans on, every row 2 cycles late, a
    fifth of the broadcasts lost, positions off by up to 3 cm, 6 cycles by step().  Per cycle, from the device's logs:
    the truth tables are the restatement's, what is seen and its age are link_oracle's on that truth, bitwise; d_agent is
    sim_oracle's on the TRUE states; every solve the oracle converges on is within X_TOL / F_TOL / S_TOL of the oracle fed
    the PERCEIVED tables (link12_oracle.solve_seen), statuses equal.  At least 90 % of the agent-cycles are compared,
    and for some of them the oracle's answer on the true tables is further than 100 X_TOL away: the link matters."""
    torch = _need_gpu()
    A, N, gait, seed, T, Ko, Kn = l12.LOOP
    state, goal, obstacles, phase = l12.head_on_team12(A, N, gait, seed)
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    tab = l12.loop_tables(A, extrapolate, p.Ts)
    r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                        obstacles=dev(torch, obstacles), plans=True, link=link_model(torch, A, tab))
    r.reset(dev(torch, state))
    cyc = []
    for c in range(T):
        r.step()
        cyc.append({k: getattr(r, k).cpu().numpy() for k in ("last_state", "plan_table", "seen_state", "seen_plan")})
        cyc[-1]["d_agent"] = r.metrics["d_agent"].cpu().numpy()
    res = host(r.results())
    assert res["link_age"].shape == (T, A) and np.array_equal(res["traj"][0], state)
    st = link_oracle.new_state(A, N, tab["max_delay"])
    m = sim_oracle.Metrics(0)
    ex = eu = es = err = 0.0
    compared = matters = differs = 0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], goal, obstacles, c, phase, gait)
        np.testing.assert_array_equal(cyc[c]["last_state"], b["last_state"], err_msg=f"cycle {c}")
        table = None
        if c:                                                   # the truth table: last cycle's plans, shifted
            table = po.shift(po.plans_of(N, res["x"][c - 1]))
            np.testing.assert_array_equal(cyc[c - 1]["plan_table"], table, err_msg=f"cycle {c}")
        seen, seen_plan, age, st = link_oracle.update(c, 0, b["last_state"], table, tab, st)
        np.testing.assert_array_equal(cyc[c]["seen_state"], seen, err_msg=f"cycle {c}")
        np.testing.assert_array_equal(res["link_age"][c], age, err_msg=f"cycle {c}")
        if c:
            np.testing.assert_array_equal(cyc[c]["seen_plan"], seen_plan, err_msg=f"cycle {c}")
        differs += not np.array_equal(seen, b["last_state"])
        m.update(c, b["com"], obstacles, b["last_state"])                       # the metrics: the truth
        np.testing.assert_array_equal(cyc[c]["d_agent"], m.d_agent, err_msg=f"cycle {c}")
        o = l12.solve_seen(p, b, seen, seen_plan)                               # the solve: what is seen
        t = l12.solve_seen(p, b, b["last_state"], table)
        err = max(err, o["line_err"], t["line_err"])
        opt = l12.converged(o["status"])
        assert np.array_equal(res["status"][c][opt], o["status"][opt]), (c, res["status"][c].tolist(), o["status"].tolist())
        compared += int(opt.sum())
        g, w = res["x"][c][opt], o["x"][opt]
        if opt.any():
            ex = max(ex, np.abs(g[:, :12 * N] - w[:, :12 * N]).max())
            eu = max(eu, np.abs(g[:, 12 * N:24 * N] - w[:, 12 * N:24 * N]).max())
            es = max(es, np.abs(g[:, -1] - w[:, -1]).max())
        both = opt & l12.converged(t["status"])
        matters += int((np.abs(o["x"][:, :12 * N] - t["x"][:, :12 * N]).max(1)[both] > 100 * X_TOL).sum())
        np.testing.assert_array_equal(res["traj"][c + 1], sim12_oracle.next_state12(res["x"][c]), err_msg=f"cycle {c}")
    np.testing.assert_array_equal(res["min_d_agent"], m.min_d_agent)
    np.testing.assert_array_equal(res["min_d_obs"], m.min_d_obs)
    print(f"{l12.LOOP}, extrapolate {extrapolate}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} "
          f"|s| {es:.3e}; the link moves {matters} of them by more than 100 X_TOL; {differs} cycles see another table "
          f"than the truth; largest age {res['link_age'].max()}; tables within {err:.1e} of their lines; min_d_agent "
          f"{res['min_d_agent'].min():.4f}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    assert matters >= 1 and err < l12.LINE_TOL
    assert differs >= 1 and res["link_age"].max() >= 2 and (res["link_age"][2:] >= 2).all()
    assert res["min_d_agent"].min() < np.sqrt(workload.EPS_NBR)                 # the inter-agent rows are active


# ================================================================================== 4. the driver against the steps
def everything(torch, mode, T=6, seed=21):
    """The head-on team with link, Plant12, plans, plan_selection and agent_rad together: host copies of results()
    and of the perceived tables."""
    A, N, gait, tseed, _, Ko, Kn = l12.LOOP
    state, goal, obstacles, phase = l12.head_on_team12(A, N, gait, tseed)
    kv, kp, kw, mass, inertia = workload.plant_tables12(A, 3)
    plant = srb12.Plant12(11, dev(torch, kv), dev(torch, kp), dev(torch, kw), dev(torch, mass), dev(torch, inertia))
    tab = l12.loop_tables(A, True, TS)
    tab["seed"] = seed
    r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                        obstacles=dev(torch, obstacles), plans=True, plan_selection=True,
                        agent_rad=dev(torch, np.full(A, 0.7)), plant=plant, link=link_model(torch, A, tab))
    r.reset(dev(torch, state))
    if mode == "run":
        r.run(T)
    else:
        for _ in range(T):
            r.step()
    out = host(r.results())
    out["seen_state"], out["seen_plan"] = r.seen_state.cpu().numpy(), r.seen_plan.cpu().numpy()
    out["plan_table"] = r.plan_table.cpu().numpy()
    return out


@gpu
def test_c_driver_equals_python_steps_bitwise_with_link_plant_plans_selection_and_agent_sizes():
    torch = _need_gpu()
    a, b = everything(torch, "run"), everything(torch, "step")
    assert sorted(a) == sorted(b) and {"disturbance", "link_age", "seen_state", "seen_plan"} <= set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    T = a["cycles"]
    assert a["link_age"].max() >= 2 and (a["disturbance"][:, :, 6] != 0).all()
    assert not np.array_equal(a["seen_state"], a["traj"][T - 1][:, [0, 1, 6, 7]])
    assert not np.array_equal(a["seen_plan"], a["plan_table"])


# ================================================================================== 5. the old paths
def plain12(torch, run, T, plans, link=None, mode="run", **kw):
    A, N, gait, seed, _, Ko, Kn = run
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                        obstacles=dev(torch, obstacles), plans=plans, plan_selection=plans, link=link, **kw)
    r.reset(dev(torch, state))
    return r


def drive_link(r, T, link):
    """T cycles of the Rollout12 r (after reset) by srb12_rollout_link_device called directly."""
    s, o = r.solver, r.out
    r._reserve(T)
    b = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], r.A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
    pl = ctypes.byref(srb12.Plans12(None, _dp(o["plan"]), 1 if r.plan_selection else 0, _dp(r.plan_table))) if r.plans else None
    srbnmpc._check(srb12._lib().srb12_rollout_link_device(s._h, r.A, ctypes.byref(b), ctypes.byref(r._sim()), pl, None, None,
                                                          None, None, None if link is None else ctypes.byref(link), T,
                                                          s._stream(None)))
    r.c, r.flushed = T, True
    return host(r.results())


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_no_link_nothing_set_and_zero_tables_are_the_plain_rollout_bitwise(plans):
    """No link, a LinkModel with nothing set, the C driver with link NULL and with a struct of NULL tables (whose seen
    and age buffers stay unwritten), and a link of zero delay and zero drop (its kernel runs): traj, x, status and every
    other output of the plain rollout, 8 agents, 5 cycles, with plans also the horizon-aware selection (whose own plan
    is then a copy of its table row).  For the first ones the solve kernel is the same."""
    torch = _need_gpu()
    run, T = sim12_oracle.RUNS12[2], 5
    A = run[0]
    r = plain12(torch, run, T, plans)
    r.run(T)
    want, kernel = host(r.results()), r.solver.last_kernel()
    assert "link_age" not in want and not np.array_equal(want["traj"][T], want["traj"][0])
    r = plain12(torch, run, T, plans, link=srbnmpc.LinkModel(seed=4))
    assert r.link is None and r.seen_state is None
    for mode in ("run", "step"):
        r = plain12(torch, run, T, plans, link=srbnmpc.LinkModel(seed=4))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        got = host(r.results())
        assert sorted(got) == sorted(want) and r.solver.last_kernel() == kernel
        for k, v in want.items():
            assert np.array_equal(got[k], v), (mode, k)
    _, age = guarded(torch, (T, A), torch.int32)
    _, seen = guarded(torch, (A, 4), torch.float64)
    empty = srbnmpc.Link(99, None, None, None, None, 2, 1, None, None, None, None, None, _dp(seen), None, _ip(age))
    for link in (None, empty):
        r = plain12(torch, run, T, plans)
        got = drive_link(r, T, link)
        assert sorted(got) == sorted(want) and r.solver.last_kernel() == kernel
        for k, v in want.items():
            assert np.array_equal(got[k], v), k
    assert (age == FILL).all() and (seen == FILL).all()
    for ext in (False, True):
        zero = srbnmpc.LinkModel(seed=4, delay=dev(torch, np.zeros(A, np.int32)), drop=dev(torch, np.zeros(A)), extrapolate=ext)
        for mode in ("run", "step"):
            r = plain12(torch, run, T, plans, link=zero)
            if mode == "run":
                r.run(T)
            else:
                for _ in range(T):
                    r.step()
            got = host(r.results())
            assert (got.pop("link_age") == 0).all()
            np.testing.assert_array_equal(r.seen_state.cpu().numpy(), want["traj"][T - 1][:, [0, 1, 6, 7]])
            for k, v in want.items():
                assert np.array_equal(got[k], v), (ext, mode, k)


# ================================================================================== 6. replicas
@gpu
def test_replicas_of_one_scene_draw_by_their_global_rows_and_the_lip_draws():
    """workload.replicate_scenes of one 4-agent make_scenes12 scene x 8 under set_scenes, plans and the plan selection
    on: with zero tables every replica is the same rollout; with noise and loss every replica has draws of its own;
    the same seed gives the same bits, another seed others.  The LIP rollout of as many rows with the same seed and
    tables loses the same messages (link_age) and, at the rows that hold a fresh message, adds the same noise draws."""
    torch = _need_gpu()
    team, n_obs, copies, N, T = 4, 5, 8, 4, 5
    sc = workload.replicate_scenes(workload.make_scenes12(1, team, N, "trot", seed=2, n_obs=n_obs), copies)
    A = team * copies
    goal = workload.cross_goals(sc["nbr_state"][:, :2], team, seed=1)
    s = srb12.Solver12(srb12.default_params(N, K_obs=1, K_nbr=2), A)
    s.set_scenes(team, n_obs)
    drop, noise = np.full(A, 0.4), np.full(A, 0.03)

    def model(seed, on):
        if not on:
            return srbnmpc.LinkModel(seed=seed, delay=dev(torch, np.zeros(A, np.int32)), drop=dev(torch, np.zeros(A)))
        return srbnmpc.LinkModel(seed=seed, drop=dev(torch, drop), noise_p=dev(torch, noise))

    def roll(seed, on):
        r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, sc["phase"]), log_x=True, obstacles=dev(torch, sc["obstacles"]),
                            plans=True, plan_selection=True, link=model(seed, on))
        r.reset(dev(torch, sc["x0"]))
        r.run(T)
        out = host(r.results())
        out["seen_state"] = r.seen_state.cpu().numpy()
        return out
    calm = roll(5, False)
    per = calm["traj"].reshape(T + 1, copies, team, 12)
    assert (calm["link_age"] == 0).all() and (per == per[:, :1]).all()
    a, again, other = roll(5, True), roll(5, True), roll(6, True)
    for k in a:
        assert np.array_equal(a[k], again[k]), k
    assert not np.array_equal(a["link_age"], other["link_age"]) and not np.array_equal(a["traj"], other["traj"])
    pa = a["traj"].reshape(T + 1, copies, team, 12)
    for i in range(copies):
        for j in range(i):
            assert not np.array_equal(pa[:, i], pa[:, j]), (i, j)
    s.close()
    rows = np.arange(A)
    truth = a["traj"][T - 1][:, [0, 1, 6, 7]]
    fresh = a["link_age"][T - 1] == 0
    u = link_oracle.draws(5, T - 1, rows, link_oracle.NOISE)
    assert fresh.any() and not fresh.all() and a["link_age"].max() >= 2
    np.testing.assert_array_equal(a["seen_state"][fresh, 0], (truth[:, 0] + noise * u[:, 0])[fresh])
    np.testing.assert_array_equal(a["seen_state"][fresh, 1], (truth[:, 1] + noise * u[:, 1])[fresh])
    # the LIP rollout of as many rows: the same losses, the same noise draws
    C = 2
    lstate, lgoal, lobs = sim_oracle.team(A, N, C, 9)
    ls = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=1, K_nbr=2), A)
    lr = srbnmpc.Rollout(ls, dev(torch, lgoal), obstacles=dev(torch, lobs), plans=True, link=model(5, True))
    lr.reset(dev(torch, lstate))
    lr.run(T)
    lres = host(lr.results())
    lseen = lr.seen_state.cpu().numpy()
    ls.close()
    assert np.array_equal(lres["link_age"], a["link_age"])
    ltruth = lres["traj"][T - 1][:, [0, 2, 1, 3]]
    np.testing.assert_array_equal(lseen[fresh, 0], (ltruth[:, 0] + noise * u[:, 0])[fresh])
    np.testing.assert_array_equal(lseen[fresh, 1], (ltruth[:, 1] + noise * u[:, 1])[fresh])


# ================================================================================== 7. refusals on a live context
@gpu
def test_refusals_by_name_on_a_live_context_and_it_survives():
    torch = _need_gpu()
    run = sim12_oracle.RUNS12[2]
    A, N, gait, seed, T, Ko, Kn = run
    r = plain12(torch, run, T, True)
    s, o = r.solver, r.out
    r._reserve(2)
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    f8 = lambda *sh: torch.zeros(sh, dtype=torch.float64, device="cuda")
    i4 = lambda *sh: torch.zeros(sh, dtype=torch.int32, device="cuda")
    D = 1
    bufs = dict(ring_state=f8(D + 1, A, 4), ring_plan=f8(D + 1, A, N, 2), held_state=f8(A, 4), held_plan=f8(A, N, 2),
                held_cycle=i4(A), seen_state=f8(A, 4), seen_plan=f8(A, N, 2))
    delay = i4(A)

    def link(**kw):
        d = dict(bufs)
        d.update(kw)
        return srbnmpc.Link(1, _ip(delay), None, None, None, D, 0, _dp(d["ring_state"]), _dp(d["ring_plan"]),
                            _dp(d["held_state"]), _dp(d["held_plan"]), _ip(d["held_cycle"]), _dp(d["seen_state"]),
                            _dp(d["seen_plan"]), None)

    def rollout(ln, b=None, pl=None):
        b = b or srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, _dp(o["x"]),
                               _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
        pl = pl or srb12.Plans12(None, _dp(o["plan"]), 1, _dp(r.plan_table))
        return lib.srb12_rollout_link_device(s._h, A, ctypes.byref(b), ctypes.byref(r._sim()), ctypes.byref(pl), None, None,
                                             None, None, ctypes.byref(ln), 1, s._stream(None))
    # the ranges that need N: the last row of seen_plan on the first of plan_table / of plans.plan
    both = f8(2 * A - 1, N, 2)
    over_table = srb12.Plans12(None, _dp(o["plan"]), 1, _dp(both[A - 1:]))
    assert rollout(link(seen_plan=both[:A]), pl=over_table) == -1 and "srb_link.seen_plan overlaps plan_table" in err()
    over_plan = srb12.Plans12(None, _dp(both[A - 1:]), 1, _dp(r.plan_table))
    assert rollout(link(seen_plan=both[:A]), pl=over_plan) == -1 and "srb_link.seen_plan overlaps srb12_plans.plan" in err()
    assert lib.srb12_link_update_device(s._h, A, ctypes.byref(link(seen_plan=both[:A])), _dp(r.last_state), _dp(both[A - 1:]),
                                        1, 0, s._stream(None)) == -1 and "srb_link.seen_plan overlaps plan_table" in err()
    assert rollout(link(seen_state=r.last_state)) == -1 and "srb_link.seen_state overlaps last_state" in err()
    assert rollout(link(ring_plan=None)) == -1 and "a plan table needs ring_plan" in err()
    shard = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 1, None, _dp(o["x"]),
                          _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
    assert rollout(link(), b=shard) == -1 and "sharded" in err()
    rad = torch.full((A,), 0.7, dtype=torch.float64, device="cuda")
    ag = srbnmpc.AgentSizes(_dp(rad), None, None, 1, None)
    b = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, _dp(o["x"]),
                      _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
    pl = srb12.Plans12(None, _dp(o["plan"]), 1, _dp(r.plan_table))
    assert lib.srb12_rollout_link_device(s._h, A, ctypes.byref(b), ctypes.byref(r._sim()), ctypes.byref(pl), None, None,
                                         ctypes.byref(ag), None, ctypes.byref(link()), 1, s._stream(None)) == -1
    assert "own_plan with srb_agent_sizes.clearance_selection = 1" in err()
    # the own plan of a solve: its range on the plan output's
    r.advance()
    out = dict(o)
    out["plan"] = both[A - 1:]
    with pytest.raises(RuntimeError, match="own_plan overlaps srb12_plans.plan"):
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, out, nbr_plan=r.plan_table,
                       plan_selection=True, own_plan=both[:A])
    with pytest.raises(RuntimeError, match="own_plan needs srb12_plans.plan_selection = 1"):
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o, nbr_plan=r.plan_table,
                       own_plan=both[:A])
    with pytest.raises(ValueError, match="own_plan must be a contiguous float64 array"):
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o, nbr_plan=r.plan_table,
                       plan_selection=True, own_plan=both[:A - 1])
    # the Python layer, by name
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    M = srbnmpc.LinkModel
    for model, word in ((M(delay=dev(torch, np.zeros(A + 1, np.int32))), "link: delay must be a contiguous"),
                        (M(drop=torch.zeros(A, dtype=torch.float64)), "link: drop must be on"),
                        (M(noise_p=dev(torch, np.full(A, -0.1))), "noise_p must be >= 0"),
                        (dict(drop=None), "link must be a srbnmpc.LinkModel")):
        with pytest.raises(ValueError, match=word):
            srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, obstacles), link=model)
    with pytest.raises(ValueError, match="link with plan_selection and nbr_clearance"):
        srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, obstacles), plans=True, plan_selection=True, agent_rad=rad,
                        nbr_clearance=True, link=M(drop=dev(torch, np.full(A, 0.2))))
    # after the refusals a plain rollout on the same context gives the bits it always gave
    rr = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, obstacles))
    rr.reset(dev(torch, state))
    rr.run(T)
    res = host(rr.results())
    want = t12.rollout12(run)
    for k in want:
        assert np.array_equal(res[k], want[k]), k
