"""GPU tests of moving obstacles in the SRB-12 mode (srb_moving through srb12_solve_batch_moving[_device],
srb12_obstacles_advance_device, srb12_rollout_moving_device; Solver12 / Rollout12 obs_vel, obs_horizon).

The device is held against the references of tests/moving12_oracle.py: with K_nbr = 0 the oracle's own answer for
the table handed over as a neighbour table, at the bounds of tests/test_srb12.py (statuses exact; X 1e-6, forces
1e-4 N, s 1e-6); with K_nbr > 0 the independent KKT certificate at the thresholds of
test_srb12_oracle_kkt_certificate (eq < 1e-9, prim < 1e-7, stat_rel < 1e-6).  Everything else is bitwise or index
for index: off is off, the rows that must not be read, the horizon-aware selection against
moving_oracle.horizon_select, the obstacle advance, the drivers against their manual loops, scenes against the
per-team runs."""
import ctypes

import numpy as np
import pytest
from conftest import converged

import moving12_oracle as mo
import moving_oracle
import plan12_oracle as po
import sim12_oracle
import sim_oracle
import srbnmpc
from srbnmpc import srb12, workload
from test_srb12 import _opt

gpu = pytest.mark.gpu
X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_srb12.py
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
OUT_KEYS = ("x_qp", "x", "obj", "status", "iters", "sel")
ROLLS = mo.RUNS0 + [sim12_oracle.RUNS12[0], sim12_oracle.RUNS12[2]]


def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, Ko, Kn, max_agents=64):
    key = (N, Ko, Kn, max_agents)
    if key not in _solvers:
        _solvers[key] = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), max_agents)
    return _solvers[key]


def nbr_of(s, b):
    return b["nbr_state"] if s.params.K_nbr > 0 else None


def host_solve(s, b, rows=slice(None), **kw):
    return s.solve(b["x0"][rows], b["xref"][rows], b["foot"][rows], b["contact"][rows], b["obstacles"], nbr_of(s, b), **kw)


def dev(torch, a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def dev_batch(torch, s, b):
    t = {k: dev(torch, b[k]) for k in ("x0", "xref", "foot", "obstacles")}
    t["nbr_state"] = dev(torch, nbr_of(s, b))
    t["contact"] = dev(torch, b["contact"], torch.int32)
    return t


def dev_out(torch, s, A, n_obs, n_all, plan=False):
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    nv, N = s.params.nv, s.params.N
    Ko, Kn = srb12.n_selected(s.params, n_obs, n_all, s.scenes)
    o = dict(x_qp=torch.full((A, nv), -7.0, **f8), x=torch.full((A, nv), -7.0, **f8), obj=torch.full((A,), -7.0, **f8),
             status=torch.full((A, 2), -7, **i4), iters=torch.full((A, 2), -7, **i4), sel=torch.full((A, Ko + Kn), -7, **i4))
    if plan:
        o["plan"] = torch.full((A, N, 2), -7.0, **f8)
    return o


def dev_solve(torch, s, b, plan=False, **kw):
    t = dev_batch(torch, s, b)
    A = b["x0"].shape[0]
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, plan)
    kw = {k: (dev(torch, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def assert_same(a, b, keys, what=""):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _hp(a):
    return None if a is None else a.ctypes.data_as(srbnmpc._dp)


def raw_host(s, b, nbr_plan, mv, with_plans):
    """srb12_solve_batch_moving itself, with host_plans and host_mv as given (None: a NULL pointer)."""
    p = s.params
    A = b["x0"].shape[0]
    arr = {k: np.ascontiguousarray(b[k], np.float64) for k in ("x0", "xref", "foot", "obstacles")}
    ct = np.ascontiguousarray(b["contact"], np.int32)
    nb = nbr_of(s, b)
    nb = None if nb is None else np.ascontiguousarray(nb, np.float64)
    Ko, Kn = srb12.n_selected(p, arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], s.scenes)
    out = dict(x_qp=np.zeros((A, p.nv)), x=np.zeros((A, p.nv)), obj=np.zeros(A), status=np.zeros((A, 2), np.int32),
               iters=np.zeros((A, 2), np.int32), sel=np.full((A, Ko + Kn), -2, np.int32), plan=np.zeros((A, p.N, 2)))
    ip = lambda a: a.ctypes.data_as(srbnmpc._ip)
    bt = srb12.Batch12(_hp(arr["x0"]), _hp(arr["xref"]), _hp(arr["foot"]), ip(ct), _hp(arr["obstacles"]), _hp(nb),
                       arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], 0, _hp(out["x_qp"]), _hp(out["x"]),
                       _hp(out["obj"]), ip(out["status"]), ip(out["iters"]), ip(out["sel"]), 0)
    pl = srb12.Plans12(_hp(nbr_plan), _hp(out["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_moving(s._h, A, ctypes.byref(bt), ctypes.byref(pl) if with_plans else None,
                                                         None if mv is None else ctypes.byref(mv)))
    return out


def raw_dev(torch, s, b, nbr_plan, mv, with_plans):
    """srb12_solve_batch_moving_device itself, plans and mv as given (None: a NULL pointer)."""
    t = dev_batch(torch, s, b)
    A = b["x0"].shape[0]
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, True)
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
    bt = srb12.Batch12(dp(t["x0"]), dp(t["xref"]), dp(t["foot"]), ip(t["contact"]), dp(t["obstacles"]), dp(t["nbr_state"]),
                       b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, 0, dp(o["x_qp"]), dp(o["x"]),
                       dp(o["obj"]), ip(o["status"]), ip(o["iters"]), ip(o["sel"]), 0)
    tab = dev(torch, nbr_plan)
    pl = srb12.Plans12(dp(tab), dp(o["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_moving_device(s._h, A, ctypes.byref(bt),
                                                                ctypes.byref(pl) if with_plans else None,
                                                                None if mv is None else ctypes.byref(mv), s._stream(None)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def batch_of(shape):
    """(N, Ko, Kn, b, w) of one of po.SHAPES12 (its K_nbr) or mo.SHAPES0 (K_nbr = 0), velocities at vmax = 1."""
    if len(shape) == 6:
        N, Ko, Kn, A, gait, seed = shape
        b = po.reference(shape)["b"]
    else:
        (N, Ko, A, gait, seed), Kn = shape, 0
        b = mo.reference(shape)["b"]
    return N, Ko, Kn, b, workload.obstacle_velocities(b["obstacles"].shape[0], seed, 1.0)


def errors(N, got, want):
    return (np.abs(got[:, :12 * N] - want[:, :12 * N]).max(), np.abs(got[:, 12 * N:24 * N] - want[:, 12 * N:24 * N]).max(),
            np.abs(got[:, -1] - want[:, -1]).max())


# ================================================================================== 1. off is off
@gpu
@pytest.mark.parametrize("shape", po.SHAPES12 + mo.SHAPES0)
def test_no_table_a_zero_table_and_a_null_struct_give_the_same_bits(shape):
    torch = _need_gpu()
    N, Ko, Kn, b, w = batch_of(shape)
    s = solver(N, Ko, Kn)
    zero = np.zeros_like(w)
    tables = [None] + ([np.array(po.reference(shape)["table"])] if Kn > 0 else [])
    for table in tables:
        kw = {} if table is None else dict(nbr_plan=table)
        plain = host_solve(s, b, **kw)                       # srb12_solve_batch_plans
        keys = OUT_KEYS + ("plan",)
        assert_same(host_solve(s, b, obs_vel=zero, **kw), plain, keys, "host, zero table")
        assert_same(raw_host(s, b, table, None, True), plain, keys, "host, mv NULL")
        assert_same(raw_host(s, b, table, srbnmpc.Moving(), True), plain, keys, "host, obs_vel NULL")
        dplain = dev_solve(torch, s, b, **kw)                # srb12_solve_batch[_plans]_device
        assert_same(dplain, plain, OUT_KEYS, "device entry vs host entry")
        assert_same(dev_solve(torch, s, b, obs_vel=zero, **kw), plain, OUT_KEYS, "device, zero table")
        assert_same(raw_dev(torch, s, b, table, None, True), plain, keys, "device, mv NULL")
        assert_same(raw_dev(torch, s, b, table, srbnmpc.Moving(), True), plain, keys, "device, obs_vel NULL")
        if table is None:                                    # plans NULL as well: srb12_solve_batch[_device]
            assert_same(raw_host(s, b, None, None, False), plain, OUT_KEYS, "host, plans NULL, mv NULL")
            assert_same(raw_dev(torch, s, b, None, None, False), plain, OUT_KEYS, "device, plans NULL, mv NULL")
            assert_same(raw_dev(torch, s, b, None, srbnmpc.Moving(_hp(None), 0, None), False), plain, OUT_KEYS, "")
    # and the table matters
    assert not np.array_equal(host_solve(s, b, obs_vel=w, **kw)["x"], plain["x"])


# ================================================================================== 2. against reference 1
@gpu
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_moving_table_against_the_oracle(shape):
    torch = _need_gpu()
    N, Ko, A, gait, seed = shape
    R = mo.reference(shape)
    b, r, w = R["b"], R["r"], np.array(R["w"])
    s = solver(N, Ko, 0)
    out = host_solve(s, b, obs_vel=w)
    assert np.array_equal(out["status"], r["status"]), (out["status"].tolist(), r["status"].tolist())
    ex, eu, es = errors(N, out["x"], r["x"])
    print(f"shape {shape}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert np.array_equal(out["sel"], mo.snapshot_select(b, b["obstacles"], Ko))
    assert_same(dev_solve(torch, s, b, obs_vel=w), out, OUT_KEYS, "device entry vs host entry")


# ================================================================================== 3. read only through sel
@gpu
@pytest.mark.parametrize("shape", mo.SHAPES0 + [po.SHAPES12[0]])
def test_the_velocity_table_is_read_only_through_sel(shape):
    torch = _need_gpu()
    N, Ko, Kn, b, w = batch_of(shape)
    s = solver(N, Ko, Kn)
    for horizon in (False, True):
        full = host_solve(s, b, obs_vel=w, obs_horizon=horizon)
        used = np.unique(full["sel"][:, :Ko])
        assert (used >= 0).all() and len(used) < w.shape[0]
        if horizon:                                          # (the horizon-aware selection scans every row)
            continue
        holes = np.full_like(w, np.nan)
        holes[used] = w[used]
        assert_same(host_solve(s, b, obs_vel=holes), full, OUT_KEYS, "host")
        assert_same(dev_solve(torch, s, b, obs_vel=holes), full, OUT_KEYS, "device")


# ================================================================================== 4. mixed shapes: the certificate
@gpu
@pytest.mark.parametrize("curved", [False, True])
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_mixed_rows_pass_the_kkt_certificate(shape, curved):
    """K_nbr > 0: the static columns move, the neighbour columns follow the constant-velocity guess or a curved plan
    table (the plans of a first solve).  Every agent converges and its point is a KKT point of the problem whose
    rows are built in numpy."""
    _need_gpu()
    N, Ko, Kn, b, w = batch_of(shape)
    A = b["x0"].shape[0]
    p = po.reference(shape)["p"]
    s = solver(N, Ko, Kn)
    table = np.ascontiguousarray(host_solve(s, b, obs_vel=w)["plan"]) if curved else None
    out = host_solve(s, b, obs_vel=w, **({} if table is None else dict(nbr_plan=table)))
    ok = _opt(out["status"])
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    for a in np.where(ok)[0]:
        obs, eps = mo.rows_moving(p, b, a, table, out["sel"][a], b["obstacles"], w)
        cert = po.certificate(p, b, a, obs, eps, out["x"][a])
        assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
    print(f"shape {shape} curved {curved}: {ok.sum()}/{A} converged, worst certificate {worst}; not converged: "
          f"{[(int(a), out['status'][a].tolist()) for a in np.where(~ok)[0]]}")
    assert ok.all(), (shape, curved, np.where(~ok)[0].tolist(), out["status"][~ok].tolist())


# ================================================================================== 5. horizon-aware selection
def _placed(b, pos, v):
    """The batch with every agent moved to pos [A][2] with CoM velocity v [A][2] (start, reference line and
    footholds shifted alike)."""
    b = {k: np.array(x) for k, x in b.items()}
    d = pos - b["x0"][:, :2]
    b["x0"][:, :2] = pos
    b["x0"][:, 6:8] = v
    b["xref"][:, :, :2] += d[:, None]
    b["foot"][:, :, :, :2] += d[:, None, None]
    b["nbr_state"] = np.ascontiguousarray(np.concatenate([pos, v], 1))
    return b


def crossing12(n_obs, A, seed, N):
    """moving_oracle's crossing world for the 12-state body: fast obstacles in a small arena, so that the order of
    approach changes over the horizon."""
    g = np.random.default_rng(seed)
    side = 1.0 + np.sqrt(n_obs)
    ob, vel = g.uniform(0, side, (n_obs, 2)), g.normal(0, 6.0, (n_obs, 2))
    pos, v = g.uniform(0, side, (A, 2)), g.normal(0, 3.0, (A, 2))
    b = _placed(workload.make_batch12(A, N, "trot", seed=seed), pos, v)
    b["obstacles"] = ob
    return b, vel


@gpu
@pytest.mark.parametrize("n_obs", [1, 3, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("Ko", [1, 3, 8])
def test_horizon_selection_index_for_index(n_obs, Ko):
    """Row counts either side of a lane, a wave and a scan pass; K_obs 1, 3, 8, and K_obs > n_obs (clamped to the rows
    that exist).  The selection is read from the solve's sel output."""
    _need_gpu()
    N, A, Kn = 4, 9, 2
    s = solver(N, Ko, Kn)
    b, vel = crossing12(n_obs, A, 1000 * Ko + n_obs, N)
    ko = min(Ko, n_obs)
    want = mo.horizon_select(s.params, b, b["obstacles"], vel, Ko)
    snap_want = mo.snapshot_select(b, b["obstacles"], Ko)
    if n_obs >= 63:
        assert (want != snap_want).any()                     # the horizon matters in this world (numpy first)
    got = host_solve(s, b, obs_vel=vel, obs_horizon=True)["sel"]
    snap = host_solve(s, b, obs_vel=vel)["sel"]
    assert got.shape == (A, ko + Kn) and want.shape == (A, ko)
    assert np.array_equal(got[:, :ko], want), np.where((got[:, :ko] != want).any(1))[0]
    assert np.array_equal(snap[:, :ko], snap_want)
    assert np.array_equal(got[:, ko:], snap[:, ko:])         # the neighbour columns are the snapshot selection's


@gpu
def test_horizon_selection_ties_nan_rows_the_1000_m_rule_and_scenes():
    torch = _need_gpu()
    N, Ko = 4, 3
    s = solver(N, Ko, 0)
    Ts = s.params.Ts
    pos = np.array([[0.0, 0.0], [2.0, 0.0]])
    b = _placed(workload.make_batch12(2, N, "stand", seed=7), pos, np.zeros((2, 2)))

    def sel_of(ob, vel):
        bb = dict(b, obstacles=ob)
        h = host_solve(s, bb, obs_vel=vel, obs_horizon=True)["sel"]
        assert np.array_equal(dev_solve(torch, s, bb, obs_vel=vel, obs_horizon=True)["sel"], h)
        return h
    # duplicate rows (1 == 2, 4 == 5): the lower index first; row 3 is far now and passes close later
    ob = np.array([[9.0, 9.0], [3.0, 4.0], [3.0, 4.0], [64.0, 1.0], [-3.0, -4.0], [-3.0, -4.0]])
    vel = np.zeros((6, 2))
    vel[3, 0] = -64.0 / (Ts * 3.0)                           # x = 0 at grid time Ts 3: distance 1
    want = mo.horizon_select(s.params, b, ob, vel, Ko)
    assert want[0].tolist() == [3, 1, 2]
    assert np.array_equal(sel_of(ob, vel), want)
    vel0 = np.zeros((6, 2))
    want0 = mo.horizon_select(s.params, b, ob, vel0, Ko)
    assert want0[0].tolist() == [1, 2, 4]
    assert np.array_equal(sel_of(ob, vel0), want0)
    # NaN in a position and in a velocity: never selected; with fewer valid rows than K_obs the rest is row 0
    obn, veln = ob.copy(), vel.copy()
    obn[1, 1] = np.nan
    veln[3, 0] = np.nan
    wantn = mo.horizon_select(s.params, b, obn, veln, Ko)
    assert wantn[0].tolist() == [2, 4, 5]
    assert np.array_equal(sel_of(obn, veln), wantn)
    obn[[2, 4, 5], 0] = np.nan
    wantn = mo.horizon_select(s.params, b, obn, veln, Ko)
    assert wantn[0].tolist() == [0, 0, 0]
    assert np.array_equal(sel_of(obn, veln), wantn)
    # an obstacle at >= 1000 m for its whole horizon gets row 0; one that comes within 1000 m is selected
    obf = np.array([[5.0, 0.0], [2000.0, 0.0], [0.0, 1500.0], [1001.0, 0.0]])
    velf = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, -1.0], [-10.0, 0.0]])
    wantf = mo.horizon_select(s.params, b, obf, velf, Ko)
    assert wantf[0].tolist() == [0, 3, 0]
    assert np.array_equal(sel_of(obf, velf), wantf)
    # 3 scenes x 4 agents x 5 obstacles, scene-major tables, global rows
    S, sa, so = 3, 4, 5
    bs, vels = crossing12(S * so, S * sa, 77, N)
    vels[7] = np.nan                                          # a NaN row of scene 1
    bs["obstacles"][10:15] += 5000.0                          # scene 2 out of reach: its row 0 is global row 10
    u = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=2), S * sa)
    try:
        u.set_scenes(sa, so)
        wants = mo.horizon_select(u.params, bs, bs["obstacles"], vels, Ko, sa, so)
        assert (wants[2 * sa:] == 10).all() and not (wants[sa:2 * sa] == 7).any()
        gots = host_solve(u, bs, obs_vel=vels, obs_horizon=True)["sel"]
        assert np.array_equal(gots[:, :Ko], wants)
        # (the neighbour columns do not depend on the table; the snapshot solve gets one without the NaN row)
        assert np.array_equal(gots[:, Ko:], host_solve(u, bs, obs_vel=np.nan_to_num(vels))["sel"][:, Ko:])
    finally:
        u.close()


# ================================================================================== 6. solve with the horizon selection
@gpu
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_solve_with_the_horizon_selection_against_the_oracle_handed_those_rows(shape):
    torch = _need_gpu()
    N, Ko, A, gait, seed = shape
    R = mo.reference(shape)
    b, p, w = R["b"], R["p"], np.array(R["w"])
    ob = b["obstacles"]
    want = mo.horizon_select(p, b, ob, w, Ko)
    x0 = np.array([po.lip_x0(x) for x in b["x0"]])
    key = moving_oracle.horizon_keys(p.Ts, N, x0, ob, w)
    assert all(len(set(r)) == Ko for r in want.tolist()) and (np.take_along_axis(key, want, 1) < 1000.0).all()
    s = solver(N, Ko, 0)
    out = host_solve(s, b, obs_vel=w, obs_horizon=True)
    assert np.array_equal(out["sel"], want)
    r = mo.solve_selected(p, b, ob, w, out["sel"])
    assert np.array_equal(out["status"], r["status"]), (out["status"].tolist(), r["status"].tolist())
    ex, eu, es = errors(N, out["x"], r["x"])
    differ = int((want != mo.snapshot_select(b, ob, Ko)).any(1).sum())
    print(f"shape {shape}: {differ} agents select other rows than now; max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert_same(dev_solve(torch, s, b, obs_vel=w, obs_horizon=True), out, OUT_KEYS, "device entry vs host entry")


# ================================================================================== 7. obstacle advance
@gpu
@pytest.mark.parametrize("n_obs", [1, 255, 256, 257])
def test_obstacle_advance_equals_numpy_bitwise(n_obs):
    torch = _need_gpu()
    s = solver(4, 1, 0)
    g = np.random.default_rng(n_obs)
    ob, vel = g.uniform(-9, 9, (n_obs, 2)), g.normal(0, 3, (n_obs, 2))
    ob[n_obs // 2, 0] = np.nan
    vel[0, 1] = np.nan
    t, v = dev(torch, ob), dev(torch, vel)
    for calls in (1, 2, 3):
        s.advance_obstacles_device(t, v)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), moving_oracle.advance_obstacles(s.params.Ts, ob, vel, calls), equal_nan=True)
    assert np.array_equal(v.cpu().numpy(), vel, equal_nan=True)


# ================================================================================== 8. rollout
_rolls = {}


def roll12(run, mode="run", plans=False, vel="table"):
    """One of ROLLS on the device with log_x, once per key: the host copies of results().  vel: "table" the run's
    velocities, "zero" a zero table, None no table."""
    key = (run, mode, plans, vel)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = run
        state, goal, ob, phase, w = mo.world12(run)
        v = None if vel is None else dev(torch, w if vel == "table" else np.zeros_like(w))
        table = dev(torch, ob)
        r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                            obstacles=table, plans=plans, obs_vel=v)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = r.results()
        torch.cuda.synchronize()
        res = host(res)
        if vel is not None:
            assert np.array_equal(table.cpu().numpy(), ob)                 # the caller's table stays
            r.reset(dev(torch, state))
            torch.cuda.synchronize()
            assert np.array_equal(r.obstacles.cpu().numpy(), ob)           # reset() restores the clone
        _rolls[key] = res
    return _rolls[key]


@gpu
@pytest.mark.parametrize("run,plans", [(r, False) for r in ROLLS] + [(r, True) for r in ROLLS if r[6] > 0])
def test_rollout_run_equals_steps_and_every_cycle_the_stand_alone_solve(run, plans):
    torch = _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    a, b = roll12(run, "run", plans), roll12(run, "step", plans)
    assert sorted(a) == sorted(b) and "obstacles" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    state, goal, ob, phase, w = mo.world12(run)
    s = solver(N, Ko, Kn)
    Ts = s.params.Ts
    assert np.array_equal(a["obstacles"], moving_oracle.advance_obstacles(Ts, ob, w, T - 1))
    assert not np.array_equal(a["obstacles"], ob)
    for c in range(T):
        assert np.array_equal(a["traj"][c + 1], a["x"][c][:, 36:48]), c
        obc = moving_oracle.advance_obstacles(Ts, ob, w, c)
        r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, (phase + c).astype(np.int32)), gait=gait,
                            obstacles=dev(torch, obc))
        r.reset(dev(torch, a["traj"][c]))
        r.advance()
        table = po.shift(po.plans_of(N, a["x"][c - 1]), 4) if plans and c > 0 else None
        o = dev_out(torch, s, A, ob.shape[0], A)
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o, obs_vel=dev(torch, w),
                       nbr_plan=dev(torch, table))
        torch.cuda.synchronize()
        got = host(o)
        assert np.array_equal(got["x"], a["x"][c]), c
        assert np.array_equal(got["status"], a["status"][c]) and np.array_equal(got["iters"], a["iters"][c]), c


@gpu
@pytest.mark.parametrize("run", ROLLS)
def test_a_zero_table_rollout_equals_the_existing_rollout(run):
    plans = run[6] > 0
    a, b = roll12(run, "run", plans, vel="zero"), roll12(run, "run", plans, vel=None)
    assert "obstacles" not in b
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(roll12(run, "run", plans)["traj"], b["traj"])   # and the table matters


@gpu
@pytest.mark.parametrize("run", [mo.RUNS0[2], sim12_oracle.RUNS12[2]])
def test_the_rollout_entry_without_a_table_is_the_entry_it_extends(run):
    """srb12_rollout_moving_device itself with mv = NULL and with a table-less srb_moving, plans NULL or given:
    the bits of srb12_rollout_device / srb12_rollout_plans_device (the existing Rollout12.run)."""
    torch = _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    state, goal, ob, phase, w = mo.world12(run)
    s = solver(N, Ko, Kn)
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
    for plans in ([False, True] if Kn > 0 else [False]):
        want = roll12(run, "run", plans, vel=None)
        for mv in (None, srbnmpc.Moving()):
            r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                                obstacles=dev(torch, ob), plans=plans)
            r.reset(dev(torch, state))
            r._reserve(T)
            o = r.out
            bt = srb12.Batch12(None, None, None, None, dp(r.obstacles), None, ob.shape[0], A, 0, None, dp(o["x"]),
                               dp(o["obj"]), ip(o["status"]), ip(o["iters"]), None, 0)
            pl = srb12.Plans12(None, dp(o["plan"]), 0, dp(r.plan_table)) if plans else None
            srbnmpc._check(srb12._lib().srb12_rollout_moving_device(
                s._h, A, ctypes.byref(bt), ctypes.byref(r._sim()), None if pl is None else ctypes.byref(pl),
                None if mv is None else ctypes.byref(mv), T, s._stream(None)))
            r.c, r.flushed = T, True
            got = r.results()
            torch.cuda.synchronize()
            got = host(got)
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (plans, mv is None, k)


@gpu
@pytest.mark.parametrize("run", mo.RUNS0)
def test_rollout_every_cycle_and_the_metrics_against_the_moving_oracle(run):
    """The rule of tests/test_rollout12_gpu.py, so that nothing drifts: the inputs of every cycle are rebuilt from the
    device's own logged state by the restatement and solved by the reference, statuses exact and x within the bounds;
    the metrics are sim_oracle.Metrics replayed on the logged trajectory and the moved table, bitwise."""
    _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    res = roll12(run)
    R = mo.closed_loop12_moving(run)
    p = R["p"]
    state, goal, ob, phase, w = mo.world12(run)
    assert np.array_equal(res["traj"][0], state)
    m = sim_oracle.Metrics(0)
    ex = eu = es = 0.0
    compared = 0
    for c in range(T):
        obc = moving_oracle.advance_obstacles(p.Ts, ob, w, c)
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], goal, obc, c, phase, gait)
        m.update(c, b["com"], obc, b["nbr_state"])
        o = mo.solve_moving(p, b, obc, w)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        both = converged(res["status"][c]) & converged(o["status"])
        compared += int(both.sum())
        if both.any():
            e = errors(N, res["x"][c][both], o["x"][both])
            ex, eu, es = max(ex, e[0]), max(eu, e[1]), max(es, e[2])
    print(f"run {run}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; min_d_obs "
          f"device smallest {res['min_d_obs'].min():.4f} median {np.median(res['min_d_obs']):.4f}, oracle-only "
          f"{R['metrics']['min_d_obs'].min():.4f} / {np.median(R['metrics']['min_d_obs']):.4f}")
    assert np.array_equal(res["status"], R["status"])
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)


# ================================================================================== 9. scenes
@gpu
@pytest.mark.parametrize("plans", [False, True])
@pytest.mark.parametrize("horizon", [False, True])
def test_scene_batched_solve_and_rollout_equal_the_per_team_runs(horizon, plans):
    """4 scenes x 4 agents x 20 obstacles: one scene-batched solve and rollout against four whole-team ones."""
    torch = _need_gpu()
    S, sa, so, N, Ko, Kn, T = 4, 4, 20, 10, 3, 3, 3
    b = workload.make_scenes12(S, sa, N, "trot", seed=21, n_obs=so)
    w = workload.obstacle_velocities(S * so, 21)
    s = solver(N, Ko, Kn)

    def team_solve(rows, obs):
        return s.solve(b["x0"][rows], b["xref"][rows], b["foot"][rows], b["contact"][rows], b["obstacles"][obs],
                       b["nbr_state"][rows], obs_vel=np.ascontiguousarray(w[obs]), obs_horizon=horizon)

    def team_roll(rows, obs, mode="run"):
        r = srb12.Rollout12(s, dev(torch, b["goal"][rows]), phase=dev(torch, b["phase"][rows]), log_x=True,
                            obstacles=dev(torch, b["obstacles"][obs]), obs_vel=dev(torch, w[obs]), obs_horizon=horizon,
                            plans=plans)
        r.reset(dev(torch, b["x0"][rows]))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = r.results()
        torch.cuda.synchronize()
        return host(res)
    parts = [(slice(i * sa, (i + 1) * sa), slice(i * so, (i + 1) * so)) for i in range(S)]
    teams = [team_solve(r, o) for r, o in parts]
    rolls = [team_roll(r, o) for r, o in parts]
    s.set_scenes(sa, so)
    try:
        out = team_solve(slice(None), slice(None))
        got = team_roll(slice(None), slice(None))
        stepped = team_roll(slice(None), slice(None), "step")
    finally:
        s.set_scenes(0, 0)
    for i, (t, (r, o)) in enumerate(zip(teams, parts)):
        for k in ("x", "x_qp", "status", "iters", "obj", "plan"):
            assert np.array_equal(out[k][r], t[k]), (i, k)
        want = t["sel"].copy()
        want[:, :Ko] = np.where(want[:, :Ko] >= 0, want[:, :Ko] + i * so, want[:, :Ko])
        want[:, Ko:] = np.where(want[:, Ko:] >= 0, want[:, Ko:] + i * sa, want[:, Ko:])
        assert np.array_equal(out["sel"][r], want), i
    for k, v in got.items():
        assert np.array_equal(v, stepped[k]), k
        if k == "cycles":
            continue
        axis = 1 if k in ("traj", "status", "iters", "x") else 0
        assert np.array_equal(v, np.concatenate([q[k] for q in rolls], axis)), k
    assert np.array_equal(got["obstacles"], moving_oracle.advance_obstacles(s.params.Ts, b["obstacles"], w, T - 1))


# ================================================================================== 10. refusals with a live context
@gpu
def test_refusals_by_name_and_the_context_survives():
    torch = _need_gpu()
    shape = mo.SHAPES0[1]
    N, Ko, A, gait, seed = shape
    R = mo.reference(shape)
    b, w = R["b"], np.array(R["w"])
    fresh = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=0), A)
    good = host_solve(fresh, b, obs_vel=w)
    fresh.close()
    s = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=0), A)
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0)
    dw = dev(torch, w)
    args = (t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], None)
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
    st = s._stream(None)

    def untouched():
        torch.cuda.synchronize()
        assert all((v == -7).all() for v in o.values())

    def refused(msg, fn):
        with pytest.raises(RuntimeError, match=msg) as e:
            fn()
        assert "srbnmpc error -1:" in str(e.value)              # SRB_ERR_ARG
        untouched()
    try:
        refused("obstacles_version", lambda: s.solve_device(*args, o, obs_vel=dw, obstacles_version=3))
        refused("horizon_selection = 1 needs obs_vel", lambda: s.solve_device(*args, o, obs_horizon=True))
        refused("horizon_selection = 1 needs obs_vel", lambda: host_solve(s, b, obs_horizon=True))
        bt = srb12.Batch12(dp(t["x0"]), dp(t["xref"]), dp(t["foot"]), ip(t["contact"]), dp(t["obstacles"]), None,
                           b["obstacles"].shape[0], 0, 0, dp(o["x_qp"]), dp(o["x"]), dp(o["obj"]), ip(o["status"]),
                           ip(o["iters"]), ip(o["sel"]), 0)
        for bad in (0, ctypes.sizeof(srbnmpc.Moving) + 8):
            mv = srbnmpc.Moving(dp(dw), 0, None); mv.struct_size = bad
            assert lib.srb12_solve_batch_moving_device(s._h, A, ctypes.byref(bt), None, ctypes.byref(mv), st) == -1
            assert "srb_moving.struct_size" in err()
        for bad in (2, -1):
            mv = srbnmpc.Moving(dp(dw), bad, None)
            assert lib.srb12_solve_batch_moving_device(s._h, A, ctypes.byref(bt), None, ctypes.byref(mv), st) == -1
            assert "horizon_selection: 0" in err()
        untouched()
        # the rollout driver
        state, goal, ob, phase = sim12_oracle.team12(A, N, gait, seed)
        wr = workload.obstacle_velocities(ob.shape[0], seed)
        r = srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, ob), obs_vel=dev(torch, wr), log_x=True)
        r.reset(dev(torch, state))
        r._reserve(2)
        ro = r.out
        for v in ro.values():
            v.fill_(-7)

        def call(mv, **kw):
            bb = srb12.Batch12(None, None, None, None, dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, dp(ro["x"]),
                               dp(ro["obj"]), ip(ro["status"]), ip(ro["iters"]), None, 0)
            for k, v in kw.items():
                setattr(bb, k, v)
            return lib.srb12_rollout_moving_device(s._h, A, ctypes.byref(bb), ctypes.byref(r._sim()), None,
                                                   ctypes.byref(mv), 1, st)
        other = r.obstacles.clone()
        assert call(srbnmpc.Moving(dp(r.obs_vel), 0, None)) == -1 and "srb_moving.obstacles missing" in err()
        assert call(srbnmpc.Moving(dp(r.obs_vel), 0, dp(other))) == -1 and "is not srb12_batch.obstacles" in err()
        assert call(srbnmpc.Moving(dp(r.obs_vel), 0, dp(r.obstacles)), obstacles_version=2) == -1
        assert "obstacles_version != 0" in err()
        assert call(srbnmpc.Moving(None, 1, dp(r.obstacles))) == -1 and "needs obs_vel" in err()
        assert call(srbnmpc.Moving(dp(r.obs_vel), 0, dp(r.obstacles)), agent_offset=1) == -1 and "sharded" in err()
        torch.cuda.synchronize()
        assert all((v == -7).all() for v in ro.values()) and np.array_equal(r.obstacles.cpu().numpy(), ob)
        with pytest.raises(ValueError, match="obs_horizon needs obs_vel"):
            srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, ob), obs_horizon=True)
        with pytest.raises(ValueError, match="obs_vel needs obstacles"):
            srb12.Rollout12(s, dev(torch, goal), obs_vel=dev(torch, wr))
        with pytest.raises(ValueError, match="obs_vel"):
            s.solve_device(*args, o, obs_vel=dw[:-1])
        # after the refusals the same objects work, with the bits of a fresh context
        r.run(2)
        res = r.results()
        torch.cuda.synchronize()
        assert res["cycles"] == 2 and res["status"].shape == (2, A, 2)
        again = host_solve(s, b, obs_vel=w)
        assert_same(again, good, OUT_KEYS + ("plan",), "after the refusals")
        assert_same(dev_solve(torch, s, b, obs_vel=w), good, OUT_KEYS, "after the refusals, device")
    finally:
        s.close()
