"""GPU tests of agent sizes in the SRB-12 mode (srb_agent_sizes through srb12_solve_batch_agents[_device],
srb12_sim_metrics_agents_device, srb12_rollout_agents_device; Solver12 / Rollout12 agent_rad, agent_pad, agent_body,
nbr_clearance).

The device is held against the references of tests/agents12_oracle.py: in its cases (a) to (d) the oracle's own answer
at the bounds of tests/test_sizes12_gpu.py (statuses exact; X 1e-6, forces 1e-4 N, s 1e-6); with drawn tables and the
other team features beside them the independent KKT certificate at the per-column levels, at the thresholds of
test_srb12_oracle_kkt_certificate (eq < 1e-9, prim < 1e-7, stat_rel < 1e-6).  Everything else is bitwise or index for
index: off is off, a uniform radius against a context created at that eps_nbr, a uniform pad against a context
created at that eps_obs, a shard against the full batch, the host path against the device path, the clearance
selection against agents_oracle.nbr_clear_select, the metrics against agents_oracle.Metrics on the com rows, the driver
against its manual loop.  The helpers are those of tests/test_moving12_gpu.py and tests/test_sizes12_gpu.py."""
import ctypes

import numpy as np
import pytest
from conftest import converged

import agents12_oracle as ao
import agents_oracle
import oracle
import plan12_oracle as po
import sim12_oracle
import srbnmpc
import test_moving12_gpu as tm
from srbnmpc import srb12, workload
from test_moving12_gpu import (OUT_KEYS, _need_gpu, assert_same, dev, dev_batch, dev_out, dev_solve, errors, host,
                               host_solve, solver)
from test_sizes12_gpu import _dp, _ip, _ref, walk
from test_srb12 import _opt

gpu = pytest.mark.gpu
X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_sizes12_gpu.py
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
AgentSizes, Sizes, Moving = srbnmpc.AgentSizes, srbnmpc.Sizes, srbnmpc.Moving
KEYS = OUT_KEYS + ("plan",)


def raw_host(s, b, nbr_plan, mv, sz, ag, with_plans, rows=slice(None), agent_offset=0):
    """srb12_solve_batch_agents itself: host_plans, host_mv, host_sz and host_ag as given (None: a NULL pointer; the
    structs are built by the caller from host arrays it keeps alive)."""
    p = s.params
    arr = {k: np.ascontiguousarray(b[k][rows], np.float64) for k in ("x0", "xref", "foot")}
    arr["obstacles"] = np.ascontiguousarray(b["obstacles"], np.float64)
    A = arr["x0"].shape[0]
    ct = np.ascontiguousarray(b["contact"][rows], np.int32)
    nb = tm.nbr_of(s, b)
    nb = None if nb is None else np.ascontiguousarray(nb, np.float64)
    Ko, Kn = srb12.n_selected(p, arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], s.scenes)
    out = dict(x_qp=np.zeros((A, p.nv)), x=np.zeros((A, p.nv)), obj=np.zeros(A), status=np.zeros((A, 2), np.int32),
               iters=np.zeros((A, 2), np.int32), sel=np.full((A, Ko + Kn), -2, np.int32), plan=np.zeros((A, p.N, 2)))
    hp, ip = tm._hp, lambda a: a.ctypes.data_as(srbnmpc._ip)
    bt = srb12.Batch12(hp(arr["x0"]), hp(arr["xref"]), hp(arr["foot"]), ip(ct), hp(arr["obstacles"]), hp(nb),
                       arr["obstacles"].shape[0], 0 if nb is None else nb.shape[0], agent_offset, hp(out["x_qp"]),
                       hp(out["x"]), hp(out["obj"]), ip(out["status"]), ip(out["iters"]), ip(out["sel"]), 0)
    pl = srb12.Plans12(hp(nbr_plan), hp(out["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_agents(s._h, A, ctypes.byref(bt), _ref(pl) if with_plans else None,
                                                         _ref(mv), _ref(sz), _ref(ag)))
    return out


def raw_dev(torch, s, b, nbr_plan, mv, sz, ag, with_plans):
    """srb12_solve_batch_agents_device itself (mv, sz and ag hold device pointers of tensors the caller keeps alive)."""
    t = dev_batch(torch, s, b)
    A = b["x0"].shape[0]
    o = dev_out(torch, s, A, b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, True)
    bt = srb12.Batch12(_dp(t["x0"]), _dp(t["xref"]), _dp(t["foot"]), _ip(t["contact"]), _dp(t["obstacles"]),
                       _dp(t["nbr_state"]), b["obstacles"].shape[0], 0 if t["nbr_state"] is None else A, 0, _dp(o["x_qp"]),
                       _dp(o["x"]), _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), _ip(o["sel"]), 0)
    tab = dev(torch, nbr_plan)
    pl = srb12.Plans12(_dp(tab), _dp(o["plan"]), 0, None)
    srbnmpc._check(srb12._lib().srb12_solve_batch_agents_device(s._h, A, ctypes.byref(bt), _ref(pl) if with_plans else None,
                                                                _ref(mv), _ref(sz), _ref(ag), s._stream(None)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_cert(p, b, a, table, sel, x, rad=None, pad=None, obs_eps=None, ob=None, w=None, g=None):
    obs, ep = ao.rows_agents(p, b, a, table, sel, rad, pad, obs_eps, ob, w, g)
    cert = po.certificate(p, b, a, obs, ep, x)
    assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
    return cert


def against(N, out, r, what):
    """Statuses exact, X / forces / s inside the bounds; the largest differences are printed."""
    assert np.array_equal(out["status"], r["status"]), (what, out["status"].tolist(), r["status"].tolist())
    ex, eu, es = errors(N, out["x"], r["x"])
    print(f"{what}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (what, ex, eu, es)
    return ex, eu, es


# ================================================================================== 1. off is off, uniform tables
@gpu
@pytest.mark.parametrize("shape", [po.SHAPES12[0], po.SHAPES12[2], po.SHAPES12[4], ao.SHAPES_D[2]])
def test_no_table_gives_the_bits_of_the_sized_entry_and_uniform_tables_those_of_a_context_at_that_level(shape):
    torch = _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    b = po.reference(shape)["b"] if Ko > 0 else ao.reference(shape, "two")["b"]
    n_obs = b["obstacles"].shape[0]
    w = workload.obstacle_velocities(n_obs, seed, 1.0)
    eps, _ = workload.obstacle_sizes(n_obs, seed)
    s = solver(N, Ko, Kn)
    dw, de = dev(torch, w), dev(torch, eps)
    r, q = ao.RAD_R, ao.PAD_Q
    u_rad = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn, eps_nbr=ao.pair_level(r, r)), A)
    u_pad = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn, eps_obs=ao.pad_level(s.params.eps_obs, q)), A)
    try:
        for vel in (None, w):
            for lev in (None, eps):
                if Ko == 0 and (vel is not None or lev is not None):
                    continue
                kv = dict(**({} if vel is None else dict(obs_vel=vel)), **({} if lev is None else dict(obs_eps=lev)))
                what = (vel is not None, lev is not None)
                plain = host_solve(s, b, **kv)               # srb12_solve_batch[_plans|_moving|_sized]
                assert_same(dev_solve(torch, s, b, **kv), plain, OUT_KEYS, ("device entry vs host entry", what))
                hmv, dmv = (None, None) if vel is None else (Moving(tm._hp(w), 0, None), Moving(_dp(dw), 0, None))
                hsz, dsz = (None, None) if lev is None else (Sizes(tm._hp(eps), None, 0), Sizes(_dp(de), None, 0))
                for ag in (None, AgentSizes()):
                    assert_same(raw_host(s, b, None, hmv, hsz, ag, True), plain, KEYS, ("host", ag is None, what))
                    assert_same(raw_dev(torch, s, b, None, dmv, dsz, ag, True), plain, KEYS, ("device", ag is None, what))
                    assert_same(raw_dev(torch, s, b, None, dmv, dsz, ag, False), plain, OUT_KEYS, ("plans NULL", what))
                # a uniform radius: the bits of a context created at eps_nbr = (r + r)^2
                want = host_solve(u_rad, b, **kv)
                got = host_solve(s, b, agent_rad=np.full(A, r), **kv)
                assert_same(got, want, KEYS, ("host, uniform rad", what))
                assert_same(dev_solve(torch, s, b, agent_rad=np.full(A, r), **kv), want, OUT_KEYS, ("device, uniform rad", what))
                assert not np.array_equal(want["x"], plain["x"])                     # and the level matters
                if Ko == 0:
                    continue
                # a uniform pad: the _mv_ instance against the default one of a context created at the padded eps_obs;
                # beside a level table, against that table padded in numpy
                kp = dict(kv)
                if lev is not None:
                    t = np.sqrt(eps) + q
                    kp["obs_eps"] = t * t
                want = host_solve(u_pad, b, **kp)
                got = host_solve(s, b, agent_pad=np.full(A, q), **kv)
                assert_same(got, want, KEYS, ("host, uniform pad", what))
                assert_same(dev_solve(torch, s, b, agent_pad=np.full(A, q), **kv), want, OUT_KEYS, ("device, uniform pad", what))
                assert not np.array_equal(want["x"], plain["x"])
    finally:
        u_rad.close()
        u_pad.close()


# ================================================================================== 2. (a) - (d) against the oracle
@gpu
@pytest.mark.parametrize("shape", ao.SHAPES12)
def test_uniform_and_per_agent_tables_against_the_oracle(shape):
    """(a) a uniform pad, (b) a uniform radius, (c) a per-agent pad table."""
    torch = _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    b = po.reference(shape)["b"]
    s = solver(N, Ko, Kn)
    for what, kw in (("pad", dict(agent_pad=np.full(A, ao.PAD_Q))), ("rad", dict(agent_rad=np.full(A, ao.RAD_R))),
                     ("pad_table", dict(agent_pad=ao.pad_table(A, seed)))):
        out = host_solve(s, b, **kw)
        against(N, out, ao.reference(shape, what), f"shape {shape} ({what})")
        assert_same(dev_solve(torch, s, b, **kw), out, OUT_KEYS, ("device entry vs host entry", what))


@gpu
@pytest.mark.parametrize("shape", ao.SHAPES_D)
def test_two_radii_table_against_the_oracle(shape):
    """(d): a two-valued radius table, K_obs = 0, the rows of the larger radius standing still."""
    torch = _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    R = ao.reference(shape, "two")
    b, rad = R["b"], np.array(R["rad"])
    s = solver(N, 0, Kn)
    out = host_solve(s, b, agent_rad=rad)
    assert np.array_equal(out["sel"], R["sel"])
    against(N, out, R["r"], f"shape {shape} (two radii)")
    assert_same(dev_solve(torch, s, b, agent_rad=rad), out, OUT_KEYS, "device entry vs host entry")
    assert not np.array_equal(out["x"], host_solve(s, b)["x"])


# ================================================================================== 3. shards, host path
@gpu
@pytest.mark.parametrize("shape", [po.SHAPES12[2], po.SHAPES12[0]])
def test_a_shard_gives_the_bits_of_the_same_agents_in_the_full_batch(shape):
    torch = _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    b = po.reference(shape)["b"]
    rad, pad, _ = workload.agent_sizes(A, seed)
    s = solver(N, Ko, Kn)
    kw = dict(agent_rad=rad, agent_pad=pad, nbr_clearance=True)
    full = host_solve(s, b, **kw)
    assert not np.array_equal(full["x"], host_solve(s, b)["x"])
    lo, hi = 3, A - 2
    rows = slice(lo, hi)
    part = host_solve(s, b, rows=rows, agent_offset=lo, **kw)
    for k in KEYS:
        assert np.array_equal(part[k], full[k][rows]), k
    # the device entry point on the shard, and the raw host entry point
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, hi - lo, b["obstacles"].shape[0], A, True)
    s.solve_device(t["x0"][rows], t["xref"][rows], t["foot"][rows], t["contact"][rows], t["obstacles"], t["nbr_state"], o,
                   agent_offset=lo, agent_rad=dev(torch, rad), agent_pad=dev(torch, pad), nbr_clearance=True)
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(o[k].cpu().numpy(), full[k][rows]), k
    ag = AgentSizes(tm._hp(rad), tm._hp(pad), None, 1, None)
    raw = raw_host(s, b, None, None, None, ag, True, rows, lo)
    for k in KEYS:
        assert np.array_equal(raw[k], full[k][rows]), k
    # the tables' own row is agent_offset + a: past the table it is refused before the launch
    with pytest.raises(RuntimeError, match="agent_offset"):
        host_solve(s, b, rows=rows, agent_offset=A - 1, **kw)
    z = solver(N, Ko, 0)
    with pytest.raises(RuntimeError, match="srb_agent_sizes: agent_offset \\+ n_agents exceeds n_all"):
        z.solve(b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], b["nbr_state"][:2], agent_pad=pad[:2])
    assert_same(host_solve(s, b, **kw), full, KEYS, "after the refusals")


# ================================================================================== 4. clearance selection
def _spread(n_all, N, seed):
    """A 12-state batch of n_all agents on a 6 m square (close enough for the radii to reorder the rows)."""
    g = np.random.default_rng(seed)
    b = workload.make_batch12(n_all, N, "stand", seed=seed, n_obs=4)
    return tm._placed(b, g.uniform(0, 6, (n_all, 2)), g.normal(0, 0.3, (n_all, 2)))


def _bent_table(p, b, seed):
    """A plan table [n_all][N][2]: the constant-velocity rows of the snapshot, each point moved by N(0, 0.5 m)."""
    t = po.cv_table(p, b["nbr_state"])
    return np.ascontiguousarray(t + np.random.default_rng(seed).normal(0, 0.5, t.shape))


@gpu
@pytest.mark.parametrize("n_all", [2, 9, 65, 130])
@pytest.mark.parametrize("Kn", [1, 3, 8])
def test_clearance_selection_index_for_index_snapshot_and_with_plans(n_all, Kn):
    _need_gpu()
    N, Ko = 4, 1
    s = solver(N, Ko, Kn, 130)
    b = _spread(n_all, N, 1000 * Kn + n_all)
    rad = np.random.default_rng(n_all + Kn).uniform(0.0, 3.0, n_all)
    kn = min(Kn, n_all - 1)
    want = ao.nbr_clear_select(b, rad, Kn)
    plain = host_solve(s, b)
    if n_all >= 9:                                            # the radii matter in this world
        assert (want != ao.nbr_clear_select(b, np.zeros(n_all), Kn)).any()
    got = host_solve(s, b, agent_rad=rad, nbr_clearance=True)["sel"]
    assert got.shape == (n_all, Ko + kn) and want.shape == (n_all, kn)
    assert np.array_equal(got[:, Ko:], want), np.where((got[:, Ko:] != want).any(1))[0]
    assert np.array_equal(got[:, :Ko], plain["sel"][:, :Ko])                        # the static columns as without
    # without nbr_clearance the radii do not touch the selection
    assert np.array_equal(host_solve(s, b, agent_rad=rad)["sel"], plain["sel"])
    # with plans the key's distance is the horizon's minimum
    table = _bent_table(s.params, b, 7)
    want_p = ao.nbr_clear_select(b, rad, Kn, plan=table)
    got_p = host_solve(s, b, agent_rad=rad, nbr_clearance=True, nbr_plan=table, plan_selection=True)["sel"]
    assert np.array_equal(got_p[:, Ko:], want_p), np.where((got_p[:, Ko:] != want_p).any(1))[0]
    if n_all >= 9:
        assert (want_p != want).any()
    # a plan table without plan_selection: the snapshot key
    got_s = host_solve(s, b, agent_rad=rad, nbr_clearance=True, nbr_plan=table)["sel"]
    assert np.array_equal(got_s[:, Ko:], want)


@gpu
def test_clearance_selection_with_scenes_minus_one_slots_and_a_nan_row():
    torch = _need_gpu()
    N, Ko, Kn = 4, 1, 3
    # 4 scenes x 4 agents, scene-major tables, global rows, snapshot and with plans
    S, sa, so_ = 4, 4, 6
    bs = workload.make_scenes12(S, sa, N, "trot", seed=21, n_obs=so_)
    rad = np.random.default_rng(5).uniform(0.0, 3.0, S * sa)
    u = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), S * sa)
    try:
        u.set_scenes(sa, so_)
        plain = host_solve(u, bs)
        want = ao.nbr_clear_select(bs, rad, Kn, scene_agents=sa)
        assert (want // sa == np.arange(S * sa)[:, None] // sa).all()
        assert (want != ao.nbr_clear_select(bs, np.zeros(S * sa), Kn, scene_agents=sa)).any()
        out = host_solve(u, bs, agent_rad=rad, nbr_clearance=True)
        assert np.array_equal(out["sel"][:, Ko:], want) and np.array_equal(out["sel"][:, :Ko], plain["sel"][:, :Ko])
        assert_same(dev_solve(torch, u, bs, agent_rad=rad, nbr_clearance=True), out, OUT_KEYS, "device vs host, scenes")
        table = _bent_table(u.params, bs, 8)
        want_p = ao.nbr_clear_select(bs, rad, Kn, plan=table, scene_agents=sa)
        assert (want_p != want).any()
        got_p = host_solve(u, bs, agent_rad=rad, nbr_clearance=True, nbr_plan=table, plan_selection=True)["sel"]
        assert np.array_equal(got_p[:, Ko:], want_p)
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        for a in np.where(_opt(out["status"]))[0]:
            check_cert(p, bs, a, None, out["sel"][a], out["x"][a], rad=rad)
    finally:
        u.close()
    # a NaN row is never selected: with 4 rows and K_nbr = 3 every other agent is left with a -1 slot, whose column
    # keeps eps_nbr (and the no-neighbour row)
    s = solver(N, Ko, Kn)
    b = _spread(4, N, 77)
    nb = np.array(b["nbr_state"])
    nb[2, 0] = np.nan
    b = dict(b, nbr_state=nb)
    rad4 = np.array([0.4, 2.5, 0.9, 0.1])
    want = ao.nbr_clear_select(b, rad4, Kn)
    assert (want[[0, 1, 3], 2] == -1).all() and not (want == 2).any() and (want[2] >= 0).all()
    out = host_solve(s, b, agent_rad=rad4, nbr_clearance=True)
    assert np.array_equal(out["sel"][:, Ko:], want)
    assert_same(dev_solve(torch, s, b, agent_rad=rad4, nbr_clearance=True), out, OUT_KEYS, "device vs host, NaN row")
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    ok = _opt(out["status"])
    assert ok[[0, 1, 3]].all(), out["status"].tolist()
    for a in (0, 1, 3):
        check_cert(p, b, a, None, out["sel"][a], out["x"][a], rad=rad4)


# ================================================================================== 5. every feature combined
@gpu
@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_drawn_tables_with_every_feature_pass_the_kkt_certificate(shape, clear):
    """Drawn rad and pad beside a drawn level table, moving obstacles and curved neighbour plans (clear: both clearance
    selections, the obstacles' over the horizon, and the plan selection)."""
    torch = _need_gpu()
    N, Ko, Kn, b, w = tm.batch_of(shape)
    A = b["x0"].shape[0]
    p = po.reference(shape)["p"]
    eps, _ = workload.obstacle_sizes(b["obstacles"].shape[0], shape[5])
    rad, pad, _ = workload.agent_sizes(A, shape[5])
    s = solver(N, Ko, Kn)
    kw = dict(obs_eps=eps, obs_vel=w, agent_rad=rad, agent_pad=pad)
    table = np.ascontiguousarray(host_solve(s, b, **kw)["plan"])
    if clear:
        kw.update(obs_clearance=True, obs_horizon=True, nbr_clearance=True, plan_selection=True)
    out = host_solve(s, b, nbr_plan=table, **kw)
    assert_same(dev_solve(torch, s, b, nbr_plan=table, **kw), out, OUT_KEYS, "device entry vs host entry")
    if clear:
        assert np.array_equal(out["sel"][:, Ko:], ao.nbr_clear_select(b, rad, Kn, plan=table))
    ok = _opt(out["status"])
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    for a in np.where(ok)[0]:
        cert = check_cert(p, b, a, table, out["sel"][a], out["x"][a], rad, pad, eps, b["obstacles"], w)
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
    print(f"shape {shape} clear {clear}: {ok.sum()}/{A} converged, worst certificate {worst}; not converged: "
          f"{[(int(a), out['status'][a].tolist()) for a in np.where(~ok)[0]]}")
    assert ok.all(), (shape, clear, np.where(~ok)[0].tolist(), out["status"][~ok].tolist())


@gpu
def test_coupled_driver_with_agent_sizes_equals_two_rounds_by_hand():
    torch = _need_gpu()
    shape = po.SHAPES12[2]
    N, Ko, Kn, b, w = tm.batch_of(shape)
    A, n_obs = b["x0"].shape[0], b["obstacles"].shape[0]
    rad, pad, _ = workload.agent_sizes(A, shape[5])
    s = solver(N, Ko, Kn)
    kw = dict(agent_rad=rad, agent_pad=pad, nbr_clearance=True)
    first = dev_solve(torch, s, b, plan=True, **kw)
    second = dev_solve(torch, s, b, plan=True, nbr_plan=first["plan"], **kw)
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, A, n_obs, A, True)
    change = s.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, outer=2,
                                    agent_rad=dev(torch, rad), agent_pad=dev(torch, pad), nbr_clearance=True)
    torch.cuda.synchronize()
    assert_same(host(o), second, KEYS, "outer = 2")
    assert change.cpu().tolist() == [np.abs(second["plan"] - first["plan"]).max()]
    assert not np.array_equal(second["x"], dev_solve(torch, s, b, plan=True, nbr_plan=first["plan"])["x"])


# ================================================================================== 6. metrics
def metrics_call(torch, s, com, ob, nbr, radius, body, cycles, collide=True):
    """srb12_sim_metrics_agents_device itself on the com rows of each cycle (radius None: no srb_sizes).  Returns the
    host copies of the outputs after the last cycle."""
    A = com[0].shape[0]
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    m = dict(d_obs=torch.full((A,), -7.0, **f8), d_agent=torch.full((A,), -7.0, **f8), min_d_obs=torch.full((A,), -7.0, **f8),
             min_d_agent=torch.full((A,), -7.0, **f8), fail_cycle=torch.full((A,), -7, **i4),
             distance_to_fail=torch.full((A,), -7.0, **f8), collide_cycle=torch.full((A,), -7, **i4))
    tob, trad, tbody = dev(torch, ob), dev(torch, radius), dev(torch, body)
    lib = srb12._lib()
    for c in range(cycles):
        tcom, tnbr = dev(torch, com[c]), dev(torch, nbr[c])
        sim = srb12.Sim12()
        sim.com, sim.obstacles, sim.nbr_state = _dp(tcom), _dp(tob), _dp(tnbr)
        sim.n_obs, sim.n_all = 0 if ob is None else ob.shape[0], A
        sim.d_obs, sim.d_agent, sim.min_d_obs, sim.min_d_agent = (_dp(m[k]) for k in ("d_obs", "d_agent", "min_d_obs",
                                                                                     "min_d_agent"))
        sim.fail_cycle, sim.distance_to_fail = _ip(m["fail_cycle"]), _dp(m["distance_to_fail"])
        sz = None if radius is None else Sizes(None, _dp(trad), 0)
        ag = None if body is None else AgentSizes(None, None, _dp(tbody), 0, _ip(m["collide_cycle"]) if collide else None)
        srbnmpc._check(lib.srb12_sim_metrics_agents_device(s._h, A, ctypes.byref(sim), _ref(sz), _ref(ag), c,
                                                           s._stream(None)))
        torch.cuda.synchronize()
    return host(m)


@gpu
@pytest.mark.parametrize("A,n_obs", [(2, 1), (9, 5), (33, 257), (70, 300)])
def test_agent_metrics_equal_the_restatement_bitwise(A, n_obs):
    torch = _need_gpu()
    s = solver(4, 1, 0, 128)
    ob, com, nbr = walk(A, n_obs, 10 * A + n_obs)
    g = np.random.default_rng(A)
    radius, body = g.uniform(0.1, 1.2, n_obs), g.uniform(0.05, 0.6, A)
    for rd in (None, radius):
        got = metrics_call(torch, s, com, ob, nbr, rd, body, 3)
        m = agents_oracle.Metrics(body, rd, 0)
        for c in range(3):
            m.update(c, com[c], ob, nbr[c])
        for k, v in m.as_dict().items():
            assert np.array_equal(got[k], v), (k, rd is None, got[k], v)
    assert (got["collide_cycle"] >= 0).any() or A < 33
    # no body table: the sized call's bits, collide_cycle untouched; a uniform body b: d_agent - (b + b)
    sized = metrics_call(torch, s, com, ob, nbr, radius, None, 3)
    assert (sized["collide_cycle"] == -7).all()
    for k in ("d_obs", "min_d_obs", "fail_cycle", "distance_to_fail"):
        assert np.array_equal(got[k], sized[k]), k
    half = metrics_call(torch, s, com, ob, nbr, radius, np.full(A, 0.25), 3, collide=False)
    assert np.array_equal(half["d_agent"], sized["d_agent"] - 0.5) and (half["collide_cycle"] == -7).all()


@gpu
def test_agent_metrics_with_scenes_equal_the_per_scene_restatement():
    torch = _need_gpu()
    S, sa, so_ = 4, 4, 6
    u = srb12.Solver12(srb12.default_params(4, K_obs=1, K_nbr=0), S * sa)
    try:
        u.set_scenes(sa, so_)
        ob, com, nbr = walk(S * sa, S * so_, 5)
        body = np.random.default_rng(3).uniform(0.05, 0.9, S * sa)
        got = metrics_call(torch, u, com, ob, nbr, None, body, 3)
        for i in range(S):
            r, o = slice(i * sa, (i + 1) * sa), slice(i * so_, (i + 1) * so_)
            m = agents_oracle.Metrics(body[r], None, 0)
            for c in range(3):
                m.update(c, com[c][r], ob[o], nbr[c][r])
            for k, v in m.as_dict().items():
                assert np.array_equal(got[k][r], v), (i, k)
    finally:
        u.close()


# ================================================================================== 7. closed loop
_rolls = {}
RUNS = [sim12_oracle.RUNS12[0], sim12_oracle.RUNS12[2]]


def run_tables(run):
    """(rad r, pad [A], body [A]) of a run: a uniform radius and a per-agent pad table, so every cycle has the oracle's
    own answer (agents12_oracle (b) and (c)); bodies twice workload.agent_sizes', large enough to touch."""
    A, N, gait, seed, T, Ko, Kn = run
    return ao.RAD_R, ao.pad_table(A, seed), 2.0 * workload.agent_sizes(A, seed)[2]


def roll(run, mode="run", tables=True):
    key = (run, mode, tables)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = run
        state, goal, ob, phase = sim12_oracle.team12(A, N, gait, seed)
        r, pad, body = run_tables(run)
        kw = dict(agent_rad=dev(torch, np.full(A, r)), agent_pad=dev(torch, pad), agent_body=dev(torch, body)) if tables else {}
        ro = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                             obstacles=dev(torch, ob), **kw)
        ro.reset(dev(torch, state))
        if mode == "run":
            ro.run(T)
        else:
            for _ in range(T):
                ro.step()
        res = ro.results()
        torch.cuda.synchronize()
        _rolls[key] = host(res)
    return _rolls[key]


@gpu
@pytest.mark.parametrize("run", RUNS)
def test_rollout_run_equals_steps_and_every_cycle_meets_the_oracle(run):
    _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    res, stepped = roll(run, "run"), roll(run, "step")
    assert sorted(res) == sorted(stepped) and "collide_cycle" in res
    for k in res:
        assert np.array_equal(res[k], stepped[k]), k
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    state, goal, ob, phase = sim12_oracle.team12(A, N, gait, seed)
    r, pad, body = run_tables(run)
    assert np.array_equal(res["traj"][0], state)
    m = agents_oracle.Metrics(body, None, 0)
    ex = eu = es = 0.0
    compared = 0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, res["traj"][c], goal, ob, c, phase, gait)
        m.update(c, b["com"], ob, b["nbr_state"])
        o = ao.solve_pad_table(p, b, pad, rad=r)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        both = converged(res["status"][c]) & converged(o["status"])
        compared += int(both.sum())
        if both.any():
            e = errors(N, res["x"][c][both], o["x"][both])
            ex, eu, es = max(ex, e[0]), max(eu, e[1]), max(es, e[2])
    print(f"run {run}: compared {compared}/{T * A} agent-cycles, max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; smallest body "
          f"clearance {res['min_d_agent'].min():.4f}, {int((res['collide_cycle'] >= 0).sum())} agents touched")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    assert compared >= 0.9 * T * A, compared
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)
    # the tables matter
    plain = roll(run, "run", tables=False)
    assert "collide_cycle" not in plain and not np.array_equal(plain["traj"], res["traj"])


def _rollout(torch, s, W, plans, tabs, nbr_clear=True):
    goal, phase, gait, ob, state, rad, pad, body = W
    kw = dict(agent_rad=dev(torch, rad), agent_pad=dev(torch, pad), agent_body=dev(torch, body),
              nbr_clearance=nbr_clear) if tabs else {}
    r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True, obstacles=dev(torch, ob),
                        plans=plans, plan_selection=plans, **kw)
    r.reset(dev(torch, state))
    return r


@gpu
@pytest.mark.parametrize("kind", ["plans", "scenes"])
def test_rollout_with_plans_and_scenes(kind):
    """One run each with drawn tables and the clearance selection: run() equals step() bitwise, every stepped cycle is
    the stand-alone agents solve and passes the certificate at the per-column levels, the metrics are the
    restatement's, and the driver with a null or empty srb_agent_sizes gives the log of the rollout without tables."""
    torch = _need_gpu()
    scenes = None
    if kind == "scenes":
        S, sa, so_, N, Ko, Kn, T, gait = 4, 4, 6, 6, 2, 2, 3, "trot"
        bs = workload.make_scenes12(S, sa, N, gait, seed=21, n_obs=so_)
        state, goal, phase, ob = bs["x0"], bs["goal"], bs["phase"], bs["obstacles"]
        seed, scenes, plans = 21, (sa, so_), False
    else:
        A, N, gait, seed, T, Ko, Kn = sim12_oracle.RUNS12[2]
        T, plans = 4, True
        state, goal, ob, phase = sim12_oracle.team12(A, N, gait, seed)
    A = state.shape[0]
    rad, pad, body = workload.agent_sizes(A, seed)
    body = 2.0 * body
    W = (goal, phase, gait, ob, state, rad, pad, body)
    s = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), A)
    try:
        if scenes:
            s.set_scenes(*scenes)
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        r = _rollout(torch, s, W, plans, True)
        drad, dpad = dev(torch, rad), dev(torch, pad)
        n_bad = 0
        worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
        for c in range(T):
            table = r.plan_table.clone() if plans and c > 0 else None
            r.step()
            o = dev_out(torch, s, A, ob.shape[0], A)
            s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o, nbr_plan=table,
                           plan_selection=table is not None, agent_rad=drad, agent_pad=dpad, nbr_clearance=True)
            torch.cuda.synchronize()
            for k in ("x", "status", "iters", "obj"):
                assert torch.equal(o[k], r.out[k]), (c, k)
            b = {k: getattr(r, k).cpu().numpy() for k in ("x0", "xref", "foot", "contact")}
            b["obstacles"], b["nbr_state"] = ob, r.last_state.cpu().numpy()
            sel, x, st = o["sel"].cpu().numpy(), o["x"].cpu().numpy(), o["status"].cpu().numpy()
            tab = None if table is None else table.cpu().numpy()
            want = ao.nbr_clear_select(b, rad, Kn, plan=tab, scene_agents=scenes[0] if scenes else 0)
            assert np.array_equal(sel[:, -want.shape[1]:], want), c
            ok = _opt(st)
            n_bad += int((~ok).sum())
            for a in np.where(ok)[0]:
                cert = check_cert(p, b, a, tab, sel[a], x[a], rad, pad)
                worst = {k: max(v, cert[k]) for k, v in worst.items()}
        res = r.results()
        torch.cuda.synchronize()
        res = host(res)
        print(f"{kind}: {T} cycles, worst certificate {worst}, {n_bad} solves not OPTIMAL")
        assert n_bad == 0
        one = _rollout(torch, s, W, plans, True)
        one.run(T)
        got = one.results()
        torch.cuda.synchronize()
        got = host(got)
        assert sorted(got) == sorted(res)
        for k in res:
            assert np.array_equal(got[k], res[k]), k
        # the metrics: agents_oracle.Metrics on the com rows, per scene with scenes
        groups = [slice(i * scenes[0], (i + 1) * scenes[0]) for i in range(A // scenes[0])] if scenes else [slice(0, A)]
        for i, rows in enumerate(groups):
            obr = ob[i * scenes[1]:(i + 1) * scenes[1]] if scenes else ob
            m = agents_oracle.Metrics(body[rows], None, 0)
            for c in range(T):
                m.update(c, sim12_oracle.com_of(res["traj"][c][rows]), obr, res["traj"][c][rows][:, [0, 1, 6, 7]])
            for k, v in m.as_dict().items():
                assert np.array_equal(res[k][rows], v), (i, k)
        if scenes:
            sr = one.scene_results()
            torch.cuda.synchronize()
            assert np.array_equal(sr["n_collided"].cpu().numpy(), (res["collide_cycle"].reshape(-1, scenes[0]) >= 0).sum(1))
            assert np.array_equal(sr["min_d_agent"].cpu().numpy(), res["min_d_agent"].reshape(-1, scenes[0]).min(1))
        # a null or empty srb_agent_sizes: the log of the rollout without tables (srb12_rollout[_plans]_device)
        base = _rollout(torch, s, W, plans, False)
        base.run(T)
        want = base.results()
        torch.cuda.synchronize()
        want = host(want)
        assert not np.array_equal(want["traj"], res["traj"])
        for ag in (None, AgentSizes()):
            raw = _rollout(torch, s, W, plans, False)
            raw._reserve(T)
            o = raw.out
            bt = srb12.Batch12(None, None, None, None, _dp(raw.obstacles), None, ob.shape[0], A, 0, None, _dp(o["x"]),
                               _dp(o["obj"]), _ip(o["status"]), _ip(o["iters"]), None, 0)
            pl = srb12.Plans12(None, _dp(o["plan"]), 1, _dp(raw.plan_table)) if plans else None
            srbnmpc._check(srb12._lib().srb12_rollout_agents_device(s._h, A, ctypes.byref(bt), ctypes.byref(raw._sim()),
                                                                    _ref(pl), None, None, _ref(ag), T, s._stream(None)))
            raw.c, raw.flushed = T, True
            rr = raw.results()
            torch.cuda.synchronize()
            rr = host(rr)
            for k in want:
                assert np.array_equal(rr[k], want[k]), (k, ag is None)
    finally:
        s.close()


# ================================================================================== 8. the Python layer with a device
@gpu
def test_rollout12_validates_the_tables_by_name_and_a_refusal_leaves_the_context_usable():
    torch = _need_gpu()
    shape = po.SHAPES12[2]
    N, Ko, Kn, A, gait, seed = shape
    b = po.reference(shape)["b"]
    rad, pad, body = workload.agent_sizes(A, seed)
    s = solver(N, Ko, Kn)
    kw = dict(agent_rad=rad, agent_pad=pad)
    good = host_solve(s, b, **kw)
    goal, ob = dev(torch, np.zeros((A, 2))), dev(torch, b["obstacles"])
    dr = dev(torch, rad)
    with pytest.raises(ValueError, match="nbr_clearance needs agent_rad"):
        srb12.Rollout12(s, goal, obstacles=ob, nbr_clearance=True)
    with pytest.raises(ValueError, match="agent_rad must be"):
        srb12.Rollout12(s, goal, obstacles=ob, agent_rad=dr[:-1])
    with pytest.raises(ValueError, match="agent_body must be"):
        srb12.Rollout12(s, goal, obstacles=ob, agent_body=dr.float())
    with pytest.raises(ValueError, match="agent_pad must be on"):
        srb12.Rollout12(s, goal, obstacles=ob, agent_pad=dr.cpu())
    with pytest.raises(ValueError, match="agent_body must be >= 0"):
        srb12.Rollout12(s, goal, obstacles=ob, agent_body=-dr)
    with pytest.raises(ValueError, match="agent_rad must be finite"):
        srb12.Rollout12(s, goal, obstacles=ob, agent_rad=dr * float("nan"))
    t = dev_batch(torch, s, b)
    o = dev_out(torch, s, A, b["obstacles"].shape[0], A)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs agent_rad") as e:
        s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, nbr_clearance=True)
    assert "srbnmpc error -1:" in str(e.value)
    torch.cuda.synchronize()
    assert all((v == -7).all() for v in o.values())
    assert_same(host_solve(s, b, **kw), good, KEYS, "after the refusals")
