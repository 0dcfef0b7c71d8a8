"""GPU tests of obstacle sizes in the SRB-12 mode (srb_sizes through srb12_solve_batch_sized[_device],
srb12_sim_metrics_sized_device, srb12_rollout_sized_device; Solver12 / Rollout12 obs_eps, obs_radius, obs_clearance).

The device is held against the references of tests/sizes12_oracle.py: with K_nbr = 0 and a two-level table the
oracle's own answer for the rows handed over at their levels, at the bounds of tests/test_srb12.py (statuses exact;
X 1e-6, forces 1e-4 N, s 1e-6); with K_nbr > 0 or a drawn table the independent KKT certificate with the gathered
levels at the thresholds of test_srb12_oracle_kkt_certificate (eq < 1e-9, prim < 1e-7, stat_rel < 1e-6).  Everything
else is bitwise or index for index: off is off, a uniform table against a context created at that level, the clearance
selection against sizes_oracle.clearance_select, the metrics against sizes_oracle.Metrics on the com rows, the driver
against its manual loop.  The helpers are those of tests/test_moving12_gpu.py."""
import ctypes

import numpy as np
import pytest
from conftest import converged

import moving12_oracle as mo
import oracle
import plan12_oracle as po
import sim12_oracle
import sim_oracle
import sizes12_oracle as so
import sizes_oracle
import srbnmpc
import test_moving12_gpu as tm
from srbnmpc import srb12, workload
from test_moving12_gpu import (OUT_KEYS, _need_gpu, assert_same, dev, dev_batch, dev_out, dev_solve, errors, host,
                               host_solve, solver)
from test_srb12 import _opt

gpu = pytest.mark.gpu
X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_srb12.py
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
Sizes = srbnmpc.Sizes

_dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
_ip = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
_ref = lambda st: None if st is None else ctypes.byref(st)


def raw_host(s, b, nbr_plan, mv, sz, with_plans):
    """srb12_solve_batch_sized itself: host_plans, host_mv and host_sz as given (None: a NULL pointer; mv and sz are
    built by the caller from host arrays it keeps alive)."""
    p = s.params
    A = b["x0"].shape[0]
    arr = {k: np.ascontiguousarray(b[k], np.float64) for k in ("x0", "xref", "foot", "obstacles")}
    ct = np.ascontiguousarray(b["contact"], np.int32)
    nb = tm.nbr_of(s, b)
    nb = None if nb is None else np.ascontiguousarray(nb, np.float64)
    Ko, Kn = srb12.n_selected(p, arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], s.scenes)
    out = dict(x_qp=np.zeros((A, p.nv)), x=np.zeros((A, p.nv)), obj=np.zeros(A), status=np.zeros((A, 2), np.int32),
               iters=np.zeros((A, 2), np.int32), sel=np.full((A, Ko + Kn), -2, np.int32), plan=np.zeros((A, p.N, 2)))
    hp, ip = tm._hp, lambda a: a.ctypes.data_as(srbnmpc._ip)
    bt = srb12.Batch12(hp(arr["x0"]), hp(arr["xref"]), hp(arr["foot"]), ip(ct), hp(arr["obstacles"]), hp(nb),
                       arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], 0, hp(out["x_qp"]), hp(out["x"]),
                       hp(out["obj"]), ip(out["status"]), ip(out["iters"]), ip(out["sel"]), 0)
    pl = srb12.Plans12(hp(nbr_plan), hp(out["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_sized(s._h, A, ctypes.byref(bt), _ref(pl) if with_plans else None,
                                                        _ref(mv), _ref(sz)))
    return out


def raw_dev(torch, s, b, nbr_plan, mv, sz, with_plans):
    """srb12_solve_batch_sized_device itself (mv and sz hold device pointers of tensors the caller keeps alive)."""
    t = dev_batch(torch, s, b)
    A = b["x0"].shape[0]
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, True)
    bt = srb12.Batch12(_dp(t["x0"]), _dp(t["xref"]), _dp(t["foot"]), _ip(t["contact"]), _dp(t["obstacles"]),
                       _dp(t["nbr_state"]), b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, 0, _dp(o["x_qp"]),
                       _dp(o["x"]), _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), _ip(o["sel"]), 0)
    tab = dev(torch, nbr_plan)
    pl = srb12.Plans12(_dp(tab), _dp(o["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_sized_device(s._h, A, ctypes.byref(bt), _ref(pl) if with_plans else None,
                                                               _ref(mv), _ref(sz), s._stream(None)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_cert(p, b, a, table, sel, eps, x, ob=None, w=None):
    obs, ep = so.rows_sized(p, b, a, table, sel, eps, ob, w)
    cert = po.certificate(p, b, a, obs, ep, x)
    assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
    return cert


# ================================================================================== 1. no table and a uniform table
@gpu
@pytest.mark.parametrize("shape", [po.SHAPES12[0], po.SHAPES12[2], po.SHAPES12[4]] + mo.SHAPES0)
def test_no_table_and_a_uniform_table_give_the_bits_of_the_entry_extended(shape):
    torch = _need_gpu()
    N, Ko, Kn, b, w = tm.batch_of(shape)
    s = solver(N, Ko, Kn)
    n_obs = b["obstacles"].shape[0]
    uni = np.full(n_obs, s.params.eps_obs)
    keys = OUT_KEYS + ("plan",)
    dw = dev(torch, w)
    tables = [None] + ([np.array(po.reference(shape)["table"])] if Kn > 0 else [])
    for table in tables:
        kw = {} if table is None else dict(nbr_plan=table)
        for vel in (None, w):
            kv = dict(kw) if vel is None else dict(kw, obs_vel=vel)
            plain = host_solve(s, b, **kv)                   # srb12_solve_batch_plans / _moving
            dplain = dev_solve(torch, s, b, **kv)            # srb12_solve_batch[_plans|_moving]_device
            assert_same(dplain, plain, OUT_KEYS, "device entry vs host entry")
            hmv = None if vel is None else srbnmpc.Moving(tm._hp(w), 0, None)
            dmv = None if vel is None else srbnmpc.Moving(_dp(dw), 0, None)
            for sz in (None, Sizes()):
                assert_same(raw_host(s, b, table, hmv, sz, True), plain, keys, ("host", sz is None))
                assert_same(raw_dev(torch, s, b, table, dmv, sz, True), plain, keys, ("device", sz is None))
                if table is None:                            # plans NULL as well
                    assert_same(raw_dev(torch, s, b, None, dmv, sz, False), plain, OUT_KEYS, "plans NULL")
            # a uniform table of eps_obs: the _mv_ instance against the default one
            assert_same(host_solve(s, b, obs_eps=uni, **kv), plain, keys, "host, uniform eps_obs")
            assert_same(dev_solve(torch, s, b, obs_eps=uni, **kv), plain, OUT_KEYS, "device, uniform eps_obs")
    # a uniform table of another level: the bits of a context created with eps_obs = e
    e = 2.75
    u = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn, eps_obs=e), b["x0"].shape[0])
    try:
        for vel in (None, w):
            kv = {} if vel is None else dict(obs_vel=vel)
            want = host_solve(u, b, **kv)
            assert_same(host_solve(s, b, obs_eps=np.full(n_obs, e), **kv), want, keys, ("host, uniform e", vel is None))
            assert_same(dev_solve(torch, s, b, obs_eps=np.full(n_obs, e), **kv), want, OUT_KEYS, "device, uniform e")
            assert not np.array_equal(want["x"], host_solve(s, b, **kv)["x"])       # and the level matters
    finally:
        u.close()


# ================================================================================== 2. two-level table, K_nbr = 0
@gpu
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_two_level_table_against_the_oracle(shape):
    torch = _need_gpu()
    N, Ko, A, gait, seed = shape
    R = so.reference(shape)
    b, r, eps = R["b"], R["r"], np.array(R["eps"])
    s = solver(N, Ko, 0)
    out = host_solve(s, b, obs_eps=eps)
    assert np.array_equal(out["sel"], R["sel"])
    assert np.array_equal(out["status"], r["status"]), (out["status"].tolist(), r["status"].tolist())
    ex, eu, es = errors(N, out["x"], r["x"])
    print(f"shape {shape}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert_same(dev_solve(torch, s, b, obs_eps=eps), out, OUT_KEYS, "device entry vs host entry")
    # the table is read only through sel
    holes = np.full_like(eps, np.nan)
    used = np.unique(out["sel"])
    holes[used] = eps[used]
    assert len(used) < len(eps)
    assert_same(host_solve(s, b, obs_eps=holes), out, OUT_KEYS, "holes")


# ================================================================================== 3. drawn table, K_nbr > 0
@gpu
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("curved", [False, True])
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_drawn_table_with_neighbours_passes_the_kkt_certificate(shape, curved, moving):
    _need_gpu()
    N, Ko, Kn, b, w = tm.batch_of(shape)
    A = b["x0"].shape[0]
    p = po.reference(shape)["p"]
    eps, _ = workload.obstacle_sizes(b["obstacles"].shape[0], shape[5])
    s = solver(N, Ko, Kn)
    kw = dict(obs_eps=eps, **(dict(obs_vel=w) if moving else {}))
    table = np.ascontiguousarray(host_solve(s, b, **kw)["plan"]) if curved else None
    out = host_solve(s, b, **kw, **({} if table is None else dict(nbr_plan=table)))
    ok = _opt(out["status"])
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    for a in np.where(ok)[0]:
        cert = check_cert(p, b, a, table, out["sel"][a], eps, out["x"][a], b["obstacles"], w if moving else None)
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
    print(f"shape {shape} curved {curved} moving {moving}: {ok.sum()}/{A} converged, worst certificate {worst}; not "
          f"converged: {[(int(a), out['status'][a].tolist()) for a in np.where(~ok)[0]]}")
    assert ok.all(), (shape, curved, moving, np.where(~ok)[0].tolist(), out["status"][~ok].tolist())


# ================================================================================== 4. clearance selection
@gpu
@pytest.mark.parametrize("n_obs", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("Ko", [1, 3, 8])
def test_clearance_selection_index_for_index_now_and_over_the_horizon(n_obs, Ko):
    _need_gpu()
    N, A, Kn = 4, 9, 2
    s = solver(N, Ko, Kn)
    b, vel = tm.crossing12(n_obs, A, 1000 * Ko + n_obs, N)
    eps = np.random.default_rng(n_obs + Ko).uniform(0.2, 9.0, n_obs)
    ko = min(Ko, n_obs)
    ob = b["obstacles"]
    want = so.clearance_select(s.params, b, ob, eps, Ko)
    want_h = so.clearance_select(s.params, b, ob, eps, Ko, vel=vel)
    if n_obs >= 64:                                           # the sizes and the horizon matter in this world
        assert (want != mo.snapshot_select(b, ob, Ko)).any() and (want_h != want).any()
        assert (want_h != mo.horizon_select(s.params, b, ob, vel, Ko)).any()
    plain = host_solve(s, b)["sel"]
    got = host_solve(s, b, obs_eps=eps, obs_clearance=True)["sel"]
    got_v = host_solve(s, b, obs_eps=eps, obs_clearance=True, obs_vel=vel)["sel"]       # no obs_horizon: the key now
    got_h = host_solve(s, b, obs_eps=eps, obs_clearance=True, obs_vel=vel, obs_horizon=True)["sel"]
    assert got.shape == (A, ko + Kn) and want.shape == (A, ko)
    assert np.array_equal(got[:, :ko], want), np.where((got[:, :ko] != want).any(1))[0]
    assert np.array_equal(got_v[:, :ko], want)
    assert np.array_equal(got_h[:, :ko], want_h), np.where((got_h[:, :ko] != want_h).any(1))[0]
    for g in (got, got_v, got_h):                            # the neighbour columns are those of the call without sizes
        assert np.array_equal(g[:, ko:], plain[:, ko:])


@gpu
def test_clearance_selection_ties_nan_negative_keys_the_1000_m_rule_and_scenes():
    torch = _need_gpu()
    N, Ko = 4, 3
    s = solver(N, Ko, 0)
    pos = np.array([[0.0, 0.0], [2.0, 0.0]])
    b = tm._placed(workload.make_batch12(2, N, "stand", seed=7), pos, np.zeros((2, 2)))

    def sel_of(ob, eps, want0):
        bb = dict(b, obstacles=ob)
        want = so.clearance_select(s.params, bb, ob, eps, Ko)
        assert want[0].tolist() == want0
        h = host_solve(s, bb, obs_eps=eps, obs_clearance=True)["sel"]
        assert np.array_equal(h, want), (h.tolist(), want.tolist())
        assert np.array_equal(dev_solve(torch, s, bb, obs_eps=eps, obs_clearance=True)["sel"], h)
    # rows 1 and 2 tie (key 3); row 3 is farther and larger (key 2); the agent stands inside row 4's level set (key
    # -1.5); row 5 has a NaN level, row 6 a negative one, row 7 is a NaN row: never selected
    ob = np.array([[9.0, 9.0], [3.0, 4.0], [3.0, 4.0], [6.0, 8.0], [0.5, 0.0], [-3.0, -4.0], [1.0, 1.0], [np.nan, 0.0]])
    eps = np.array([1.0, 4.0, 4.0, 64.0, 4.0, np.nan, -1.0, 1.0])
    sel_of(ob, eps, [4, 3, 1])
    sel_of(ob[[0, 1, 2, 5, 6, 7]], eps[[0, 1, 2, 5, 6, 7]], [1, 2, 0])
    # fewer valid rows than K_obs: the rest is row 0
    eps2 = eps.copy()
    eps2[[0, 1, 2, 3]] = np.nan
    sel_of(ob, eps2, [4, 0, 0])
    # every key at or beyond 1000: row 0 in every slot; a body large enough to come within 1000 m is selected
    obf = np.array([[5000.0, 0.0], [0.0, 2000.0], [-3000.0, 0.0], [1500.0, 0.0]])
    sel_of(obf, np.ones(4), [0, 0, 0])
    sel_of(obf, np.array([1.0, 1.0, 1.0, 600.0 ** 2]), [3, 0, 0])
    # 4 scenes x 4 agents x 6 obstacles, scene-major tables, global rows, now and over the horizon
    S, sa, so_ = 4, 4, 6
    bs = workload.make_scenes12(S, sa, N, "trot", seed=21, n_obs=so_)
    epss, _ = workload.obstacle_sizes(S * so_, 21)
    vels = workload.obstacle_velocities(S * so_, 21, 3.0)
    epss[7] = np.nan                                           # a NaN level in scene 1
    bs["obstacles"][12:18] += 5000.0                           # scene 2 out of reach: its row 0 is global row 12
    u = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=2), S * sa)
    try:
        u.set_scenes(sa, so_)
        plain = host_solve(u, bs)["sel"]
        for kw, vel in ((dict(), None), (dict(obs_vel=vels, obs_horizon=True), vels)):
            want = so.clearance_select(u.params, bs, bs["obstacles"], epss, Ko, vel=vel, scene_agents=sa, scene_obs=so_)
            assert (want[2 * sa:3 * sa] == 12).all() and not (want[sa:2 * sa] == 7).any()
            got = host_solve(u, bs, obs_eps=epss, obs_clearance=True, **kw)["sel"]
            assert np.array_equal(got[:, :Ko], want)
            assert np.array_equal(got[:, Ko:], plain[:, Ko:])
            assert np.array_equal(dev_solve(torch, u, bs, obs_eps=epss, obs_clearance=True, **kw)["sel"], got)
    finally:
        u.close()


@gpu
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_solve_with_the_clearance_selection_against_the_oracle_handed_those_rows(shape):
    torch = _need_gpu()
    N, Ko, A, gait, seed = shape
    R = so.reference(shape)
    b, p, eps = R["b"], R["p"], np.array(R["eps"])
    ob = b["obstacles"]
    want = so.clearance_select(p, b, ob, eps, Ko)
    assert all(len(set(r)) == Ko for r in want.tolist())
    s = solver(N, Ko, 0)
    out = host_solve(s, b, obs_eps=eps, obs_clearance=True)
    assert np.array_equal(out["sel"], want)
    r = so.solve_two_level(p, b, ob, eps, out["sel"])
    assert np.array_equal(out["status"], r["status"]), (out["status"].tolist(), r["status"].tolist())
    ex, eu, es = errors(N, out["x"], r["x"])
    differ = int((want != R["sel"]).any(1).sum())
    print(f"shape {shape}: {differ} agents select other rows than by centre; max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert_same(dev_solve(torch, s, b, obs_eps=eps, obs_clearance=True), out, OUT_KEYS, "device entry vs host entry")


# ================================================================================== 5. metrics
def metrics_call(torch, s, com, ob, nbr, radius, cycles):
    """srb12_sim_metrics[_sized]_device itself on the com rows of each cycle (radius None: the plain entry point).
    Returns the host copies of the six outputs after the last cycle."""
    A = com[0].shape[0]
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    m = dict(d_obs=torch.full((A,), -7.0, **f8), d_agent=torch.full((A,), -7.0, **f8), min_d_obs=torch.full((A,), -7.0, **f8),
             min_d_agent=torch.full((A,), -7.0, **f8), fail_cycle=torch.full((A,), -7, **i4),
             distance_to_fail=torch.full((A,), -7.0, **f8))
    tob, trad = dev(torch, ob), dev(torch, radius)
    lib = srb12._lib()
    for c in range(cycles):
        tcom, tnbr = dev(torch, com[c]), dev(torch, nbr[c])
        sim = srb12.Sim12()
        sim.com, sim.obstacles, sim.nbr_state = _dp(tcom), _dp(tob), _dp(tnbr)
        sim.n_obs, sim.n_all = 0 if ob is None else ob.shape[0], A
        sim.d_obs, sim.d_agent, sim.min_d_obs, sim.min_d_agent = (_dp(m[k]) for k in ("d_obs", "d_agent", "min_d_obs",
                                                                                     "min_d_agent"))
        sim.fail_cycle, sim.distance_to_fail = _ip(m["fail_cycle"]), _dp(m["distance_to_fail"])
        if radius is None:
            srbnmpc._check(lib.srb12_sim_metrics_device(s._h, A, ctypes.byref(sim), c, s._stream(None)))
        else:
            sz = Sizes(None, _dp(trad), 0)
            srbnmpc._check(lib.srb12_sim_metrics_sized_device(s._h, A, ctypes.byref(sim), ctypes.byref(sz), c,
                                                              s._stream(None)))
        torch.cuda.synchronize()
    return host(m)


def walk(A, n_obs, seed, cycles=3):
    """com rows [cycles][A][4] of agents walking through n_obs obstacles, and the matching snapshot rows."""
    g = np.random.default_rng(seed)
    ob = g.uniform(0, 6, (n_obs, 2))
    p0, v = g.uniform(0, 6, (A, 2)), g.normal(0, 1.5, (A, 2))
    com = [np.stack([p0[:, 0] + c * v[:, 0], v[:, 0], p0[:, 1] + c * v[:, 1], v[:, 1]], 1) for c in range(cycles)]
    nbr = [np.ascontiguousarray(q[:, [0, 2, 1, 3]]) for q in com]
    return ob, com, nbr


@gpu
@pytest.mark.parametrize("A,n_obs", [(1, 1), (9, 5), (33, 257), (70, 300)])
def test_sized_metrics_equal_the_restatement_bitwise(A, n_obs):
    torch = _need_gpu()
    s = solver(4, 1, 0, 128)
    ob, com, nbr = walk(A, n_obs, 10 * A + n_obs)
    radius = np.random.default_rng(A).uniform(0.1, 1.2, n_obs)
    radius[n_obs // 2] = np.nan                                # a NaN term never wins
    got = metrics_call(torch, s, com, ob, nbr, radius, 3)
    m = sizes_oracle.Metrics(radius, 0)
    for c in range(3):
        m.update(c, com[c], ob, nbr[c])
    for k, v in m.as_dict().items():
        assert np.array_equal(got[k], v), (k, got[k], v)
    assert (got["fail_cycle"] >= 0).any() or n_obs < 257
    # a uniform 0.5 table: d_obs - 0.5 and the fail_cycle of srb12_sim_metrics_device
    plain = metrics_call(torch, s, com, ob, nbr, None, 3)
    half = metrics_call(torch, s, com, ob, nbr, np.full(n_obs, 0.5), 3)
    assert np.array_equal(half["d_obs"], plain["d_obs"] - 0.5) and np.array_equal(half["min_d_obs"], plain["min_d_obs"] - 0.5)
    for k in ("fail_cycle", "distance_to_fail", "d_agent", "min_d_agent"):
        assert np.array_equal(half[k], plain[k]), k
    # an empty table gives +inf; a table of NaN radii as well
    none = metrics_call(torch, s, com, None, nbr, np.zeros(1), 2)
    assert np.isposinf(none["d_obs"]).all() and (none["fail_cycle"] == -1).all()
    nan = metrics_call(torch, s, com, ob, nbr, np.full(n_obs, np.nan), 2)
    assert np.isposinf(nan["d_obs"]).all() and (nan["fail_cycle"] == -1).all()


@gpu
def test_sized_metrics_with_scenes_equal_the_per_scene_restatement():
    torch = _need_gpu()
    S, sa, so_ = 4, 4, 6
    u = srb12.Solver12(srb12.default_params(4, K_obs=1, K_nbr=0), S * sa)
    try:
        u.set_scenes(sa, so_)
        ob, com, nbr = walk(S * sa, S * so_, 5)
        radius = np.random.default_rng(3).uniform(0.1, 1.5, S * so_)
        got = metrics_call(torch, u, com, ob, nbr, radius, 3)
        for i in range(S):
            r, o = slice(i * sa, (i + 1) * sa), slice(i * so_, (i + 1) * so_)
            m = sizes_oracle.Metrics(radius[o], 0)
            for c in range(3):
                m.update(c, com[c][r], ob[o], nbr[c][r])
            for k, v in m.as_dict().items():
                assert np.array_equal(got[k][r], v), (i, k)
    finally:
        u.close()


# ================================================================================== 6. rollout
_rolls = {}


def roll(run, mode="run", sized=True, radius=True):
    """One of mo.RUNS0 on the device with log_x and the run's two-level table, once per key."""
    key = (run, mode, sized, radius)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = run
        state, goal, ob, phase, w = mo.world12(run)
        eps, rad = so.two_level_table(ob.shape[0], seed)
        r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                            obstacles=dev(torch, ob), obs_eps=dev(torch, eps) if sized else None,
                            obs_radius=dev(torch, rad) if sized and radius else None)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = r.results()
        torch.cuda.synchronize()
        _rolls[key] = host(res)
    return _rolls[key]


@gpu
@pytest.mark.parametrize("run", mo.RUNS0)
def test_rollout_run_equals_steps_and_every_cycle_meets_the_two_level_reference(run):
    _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    res, stepped = roll(run, "run"), roll(run, "step")
    assert sorted(res) == sorted(stepped)
    for k in res:
        assert np.array_equal(res[k], stepped[k]), k
    p = oracle.params12(N, K_obs=Ko, K_nbr=0)
    state, goal, ob, phase, w = mo.world12(run)
    eps, rad = so.two_level_table(ob.shape[0], seed)
    assert np.array_equal(res["traj"][0], state)
    m = sizes_oracle.Metrics(rad, 0)
    ex = eu = es = 0.0
    compared = 0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], goal, ob, c, phase, gait)
        m.update(c, b["com"], ob, b["nbr_state"])
        o = so.solve_two_level(p, b, ob, eps, mo.snapshot_select(b, ob, Ko))
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        both = converged(res["status"][c]) & converged(o["status"])
        compared += int(both.sum())
        if both.any():
            e = errors(N, res["x"][c][both], o["x"][both])
            ex, eu, es = max(ex, e[0]), max(eu, e[1]), max(es, e[2])
    print(f"run {run}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; clearance to "
          f"the bodies smallest {res['min_d_obs'].min():.4f} median {np.median(res['min_d_obs']):.4f}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)
    # the levels matter, and obs_radius alone changes the metrics only
    plain = roll(run, "run", sized=False)
    assert not np.array_equal(plain["traj"], res["traj"])
    no_rad = roll(run, "run", radius=False)
    assert np.array_equal(no_rad["traj"], res["traj"]) and np.array_equal(no_rad["x"], res["x"])
    m0 = sim_oracle.Metrics(0)
    for c in range(T):
        m0.update(c, sim12_oracle.com_of(res["traj"][c]), ob, res["traj"][c][:, [0, 1, 6, 7]])
    for k, v in m0.as_dict().items():
        assert np.array_equal(no_rad[k], v), k


def stepped_world(torch, s, W, T, plans=False, vel=None, clearance=False):
    """A Rollout12 over the world W (goal, phase, gait, ob, state, eps, rad) stepped T cycles; after every step the
    stand-alone sized solve on the rollout's own inputs must give the rollout's bits, and its sel serves the
    certificate.  Returns (the host results, the per-cycle list of (b, table, sel, x, status, obstacles))."""
    goal, phase, gait, ob, state, eps, rad = W
    A, N = state.shape[0], s.params.N
    deps, dvel = dev(torch, eps), dev(torch, vel)
    r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, ob),
                        plans=plans, obs_vel=dvel, obs_horizon=vel is not None and clearance, obs_eps=deps,
                        obs_radius=dev(torch, rad), obs_clearance=clearance)
    r.reset(dev(torch, state))
    cycles = []
    for c in range(T):
        table = r.plan_table.clone() if plans and c > 0 else None
        r.step()
        o = dev_out(torch, s, A, ob.shape[0], A)
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o, nbr_plan=table, obs_vel=dvel,
                       obs_horizon=r.obs_horizon, obs_eps=deps, obs_clearance=clearance)
        torch.cuda.synchronize()
        for k in ("x", "status", "iters", "obj"):
            assert torch.equal(o[k], r.out[k]), (c, k)
        b = {k: getattr(r, k).cpu().numpy() for k in ("x0", "xref", "foot", "contact")}
        b["obstacles"], b["nbr_state"] = r.obstacles.cpu().numpy(), r.last_state.cpu().numpy()
        cycles.append((b, None if table is None else table.cpu().numpy(), o["sel"].cpu().numpy(), o["x"].cpu().numpy(),
                       o["status"].cpu().numpy(), b["obstacles"]))
    res = r.results()
    torch.cuda.synchronize()
    return host(res), cycles, r


def run_world(torch, s, W, T, plans=False, vel=None, clearance=False, sz="given", mv="given"):
    """srb12_rollout_sized_device in one call: through Rollout12.run, or (sz / mv None or a table-less struct) raw."""
    goal, phase, gait, ob, state, eps, rad = W
    A = state.shape[0]
    tabs = sz == "given"
    r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, ob),
                        plans=plans, obs_vel=dev(torch, vel), obs_horizon=vel is not None and clearance,
                        obs_eps=dev(torch, eps) if tabs else None, obs_radius=dev(torch, rad) if tabs else None,
                        obs_clearance=clearance and tabs)
    r.reset(dev(torch, state))
    if tabs:
        r.run(T)
    else:
        r._reserve(T)
        o = r.out
        bt = srb12.Batch12(None, None, None, None, _dp(r.obstacles), None, ob.shape[0], A, 0, None, _dp(o["x"]),
                           _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
        pl = srb12.Plans12(None, _dp(o["plan"]), 0, _dp(r.plan_table)) if plans else None
        m = r._moving() if vel is not None else mv
        srbnmpc._check(srb12._lib().srb12_rollout_sized_device(s._h, A, ctypes.byref(bt), ctypes.byref(r._sim()), _ref(pl),
                                                               _ref(m), _ref(sz), T, s._stream(None)))
        r.c, r.flushed = T, True
    res = r.results()
    torch.cuda.synchronize()
    return host(res)


def certify_cycles(p, cycles, eps, vel=None):
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    n = 0
    for b, table, sel, x, status, obc in cycles:
        ok = _opt(status)
        n += int((~ok).sum())
        for a in np.where(ok)[0]:
            cert = check_cert(p, b, a, table, sel[a], eps, x[a], obc, vel)
            worst = {k: max(v, cert[k]) for k, v in worst.items()}
    return worst, n


@gpu
@pytest.mark.parametrize("kind", ["plans", "moving", "scenes"])
def test_rollout_with_plans_moving_obstacles_and_scenes(kind):
    """One run each: run() equals step() bitwise, every stepped cycle is the stand-alone sized solve and passes the
    certificate with the gathered levels, the metrics are the restatement's, and the driver with null tables gives
    the log of the rollout without tables."""
    torch = _need_gpu()
    vel, scenes, plans, clearance = None, None, False, False
    if kind == "scenes":
        S, sa, so_, N, Ko, Kn, T, gait = 4, 4, 6, 6, 2, 2, 3, "trot"
        bs = workload.make_scenes12(S, sa, N, gait, seed=21, n_obs=so_)
        state, goal, phase, ob = bs["x0"], bs["goal"], bs["phase"], bs["obstacles"]
        eps, rad = workload.obstacle_sizes(S * so_, 21)
        scenes, clearance = (sa, so_), True
    else:
        run = sim12_oracle.RUNS12[2] if kind == "plans" else mo.RUNS0[2]
        A, N, gait, seed, T, Ko, Kn = run
        T = 4
        state, goal, ob, phase, w = mo.world12(run)
        eps, rad = workload.obstacle_sizes(ob.shape[0], seed)
        plans, vel = kind == "plans", (w if kind == "moving" else None)
        clearance = kind == "moving"
    W = (goal, phase, gait, ob, state, eps, rad)
    s = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), state.shape[0])
    try:
        if scenes:
            s.set_scenes(*scenes)
        res, cycles, r = stepped_world(torch, s, W, T, plans, vel, clearance)
        one = run_world(torch, s, W, T, plans, vel, clearance)
        assert sorted(one) == sorted(res)
        for k in res:
            assert np.array_equal(one[k], res[k]), k
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        worst, n_bad = certify_cycles(p, cycles, eps, vel)
        print(f"{kind}: {T} cycles, worst certificate {worst}, {n_bad} solves not OPTIMAL")
        assert n_bad == 0
        if scenes:
            sr = r.scene_results()
            torch.cuda.synchronize()
            assert sr["n_scenes"] == 4
            assert np.array_equal(sr["min_d_obs"].cpu().numpy(), res["min_d_obs"].reshape(4, 4).min(1))
            assert np.array_equal(sr["n_failed"].cpu().numpy(), (res["fail_cycle"].reshape(4, 4) >= 0).sum(1))
            sa, so_ = scenes
            for i in range(4):
                rows, o = slice(i * sa, (i + 1) * sa), slice(i * so_, (i + 1) * so_)
                m = sizes_oracle.Metrics(rad[o], 0)
                for c in range(T):
                    m.update(c, sim12_oracle.com_of(res["traj"][c][rows]), ob[o], res["traj"][c][rows][:, [0, 1, 6, 7]])
                for k, v in m.as_dict().items():
                    assert np.array_equal(res[k][rows], v), (i, k)
        else:
            m = sizes_oracle.Metrics(rad, 0)
            for c in range(T):
                m.update(c, sim12_oracle.com_of(res["traj"][c]), cycles[c][5], res["traj"][c][:, [0, 1, 6, 7]])
            for k, v in m.as_dict().items():
                assert np.array_equal(res[k], v), k
        # null tables: the log of the rollout without tables (srb12_rollout[_plans|_moving]_device)
        want = run_world(torch, s, W, T, plans, vel, False, sz=None, mv=None)
        again = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                                obstacles=dev(torch, ob), plans=plans, obs_vel=dev(torch, vel))
        again.reset(dev(torch, state))
        again.run(T)
        base = again.results()
        torch.cuda.synchronize()
        base = host(base)
        for k in base:
            assert np.array_equal(want[k], base[k]), k
        for sz, mv in ((Sizes(), None), (Sizes(), srbnmpc.Moving())):
            got = run_world(torch, s, W, T, plans, vel, False, sz=sz, mv=mv)
            for k in base:
                assert np.array_equal(got[k], base[k]), k
        assert not np.array_equal(base["traj"], res["traj"])
    finally:
        s.close()


# ================================================================================== 7. coupled driver
@gpu
def test_coupled_driver_with_sizes_equals_two_rounds_by_hand():
    torch = _need_gpu()
    shape = po.SHAPES12[2]
    N, Ko, Kn, b, w = tm.batch_of(shape)
    A, n_obs = b["x0"].shape[0], b["obstacles"].shape[0]
    eps, _ = workload.obstacle_sizes(n_obs, shape[5])
    s = solver(N, Ko, Kn)
    first = dev_solve(torch, s, b, plan=True, obs_eps=eps, obs_clearance=True)
    second = dev_solve(torch, s, b, plan=True, obs_eps=eps, obs_clearance=True, nbr_plan=first["plan"])
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, A, n_obs, A, True)
    change = s.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, outer=2,
                                    obs_eps=dev(torch, eps), obs_clearance=True)
    torch.cuda.synchronize()
    assert_same(host(o), second, OUT_KEYS + ("plan",), "outer = 2")
    assert change.cpu().tolist() == [np.abs(second["plan"] - first["plan"]).max()]
    assert not np.array_equal(second["x"], dev_solve(torch, s, b, plan=True, nbr_plan=first["plan"])["x"])


# ================================================================================== 8. the Python layer with a device
@gpu
def test_rollout12_validates_the_tables_by_name_and_a_refusal_leaves_the_context_usable():
    torch = _need_gpu()
    shape = mo.SHAPES0[1]
    N, Ko, A, gait, seed = shape
    R = so.reference(shape)
    b, eps = R["b"], np.array(R["eps"])
    s = solver(N, Ko, 0)
    good = host_solve(s, b, obs_eps=eps)
    goal, ob = dev(torch, np.zeros((A, 2))), dev(torch, b["obstacles"])
    de = dev(torch, eps)
    with pytest.raises(ValueError, match="obs_clearance needs obs_eps"):
        srb12.Rollout12(s, goal, obstacles=ob, obs_clearance=True)
    with pytest.raises(ValueError, match="obs_radius needs obstacles"):
        srb12.Rollout12(s, goal, obs_radius=de)
    with pytest.raises(ValueError, match="obs_eps needs obstacles"):
        srb12.Rollout12(s, goal, obs_eps=de)
    with pytest.raises(ValueError, match="obs_eps must be"):
        srb12.Rollout12(s, goal, obstacles=ob, obs_eps=de[:-1])
    with pytest.raises(ValueError, match="obs_radius must be"):
        srb12.Rollout12(s, goal, obstacles=ob, obs_radius=de.float())
    with pytest.raises(ValueError, match="obs_eps must be on"):
        srb12.Rollout12(s, goal, obstacles=ob, obs_eps=de.cpu())
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs obs_eps") as e:
        s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], None, o, obs_clearance=True)
    assert "srbnmpc error -1:" in str(e.value)
    torch.cuda.synchronize()
    assert all((v == -7).all() for v in o.values())
    assert_same(host_solve(s, b, obs_eps=eps), good, OUT_KEYS + ("plan",), "after the refusals")
