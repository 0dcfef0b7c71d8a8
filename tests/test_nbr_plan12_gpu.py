"""GPU tests of the neighbour plans of the SRB-12 mode (srb12_plans; srb12_solve_batch_plans[_device],
srb12_shift_plans_device, srb12_rollout_plans_device; Solver12 / Rollout12).

No oracle answers an arbitrary plan table (orc12_solve_agent predicts the neighbours itself), so the device is held
against the two references of tests/plan12_oracle.py: for linear tables the oracle's answer for the snapshot whose
velocities draw the same table, at the bounds of test_srb12_gpu_vs_oracle (statuses exact; X 1e-6, forces 1e-4 N,
s 1e-6); for curved tables the independent KKT certificate at the thresholds of test_srb12_oracle_kkt_certificate
(eq < 1e-9, prim < 1e-7, stat_rel < 1e-6).  Everything else is bitwise: the constant-velocity table against the
plain solve, the rows that must not be read, the plan output, shards, scenes, the shift kernel against
dist.shift_plans, the drivers against their manual loops."""
import ctypes

import numpy as np
import pytest

import oracle
import plan12_oracle as po
import sim12_oracle
import sim_oracle
import srbnmpc
from srbnmpc import dist as sdist
from srbnmpc import srb12, workload
from test_nbr_plan import brute_force
from test_srb12 import _opt, _rejected_polish_batch

gpu = pytest.mark.gpu
X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_srb12.py
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
OUT_KEYS = ("x_qp", "x", "obj", "status", "iters", "sel")


def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, Ko, Kn, max_agents=64, **kw):
    key = (N, Ko, Kn, max_agents, tuple(sorted(kw.items())))
    if key not in _solvers:
        _solvers[key] = srb12.Solver12(srb12.default_params(N, K_obs=Ko, K_nbr=Kn, **kw), max_agents)
    return _solvers[key]


def host_solve(s, b, rows=slice(None), **kw):
    return s.solve(b["x0"][rows], b["xref"][rows], b["foot"][rows], b["contact"][rows], b["obstacles"], b["nbr_state"], **kw)


def dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def dev_batch(torch, b):
    t = {k: dev(torch, b[k]) for k in ("x0", "xref", "foot", "obstacles", "nbr_state")}
    t["contact"] = dev(torch, b["contact"], torch.int32)
    return t


def dev_out(torch, s, A, n_obs, n_all, plan=True):
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    nv, N = s.params.nv, s.params.N
    Ko, Kn = srb12.n_selected(s.params, n_obs, n_all, s.scenes)
    o = dict(x_qp=torch.zeros((A, nv), **f8), x=torch.zeros((A, nv), **f8), obj=torch.zeros(A, **f8),
             status=torch.zeros((A, 2), **i4), iters=torch.zeros((A, 2), **i4), sel=torch.full((A, Ko + Kn), -7, **i4))
    if plan:
        o["plan"] = torch.full((A, N, 2), -7.0, **f8)
    return o


def dev_solve(torch, s, t, o, **kw):
    s.solve_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def assert_same(a, b, keys, what=""):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def certified(p, b, a, table, sel, x):
    obs, eps = po.rows(p, b, a, table, sel=sel)
    cert = po.certificate(p, b, a, obs, eps, x)
    assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
    return cert


# ================================================================================== 1. linear tables vs the oracle
@gpu
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_linear_tables_against_the_oracle(shape):
    _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    p, b, r = R["p"], R["b"], R["r_lin"]
    s = solver(N, Ko, Kn)
    out = host_solve(s, b, nbr_plan=np.array(R["table"]))
    assert (out["status"] == r["status"]).all(), (out["status"].tolist(), r["status"].tolist())
    ex = np.abs(out["x"][:, :12 * N] - r["x"][:, :12 * N]).max()
    eu = np.abs(out["x"][:, 12 * N:24 * N] - r["x"][:, 12 * N:24 * N]).max()
    es = np.abs(out["x"][:, -1] - r["x"][:, -1]).max()
    print(f"shape {shape}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}")
    assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
    # (the neighbour columns clamp to the A - 1 rows that exist; the oracle fills the rest with -1)
    want = np.array([po.select(p, b, a) for a in range(A)])
    kn = min(Kn, A - 1)
    assert np.array_equal(out["sel"], want[:, :Ko + kn]) and (want[:, Ko + kn:] == -1).all()
    assert np.array_equal(out["plan"], po.plans_of(N, out["x"]))


# ================================================================================== 2. the constant-velocity table
@gpu
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_constant_velocity_table_equals_the_plain_solve(shape):
    """The table p + v * (Ts (k + 1)) built in numpy gives the bits of the solve without a table: the kernel's own
    prediction is that expression, neither side contracted to an fma."""
    _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    s = solver(N, Ko, Kn)
    plain = host_solve(s, R["b"])
    cv = host_solve(s, R["b"], nbr_plan=po.cv_table(R["p"], R["b"]["nbr_state"]))
    d = np.abs(cv["x"] - plain["x"]).max()
    print(f"shape {shape}: max |x(cv table) - x(no table)| = {d:.3e}")
    assert_same(cv, plain, OUT_KEYS + ("plan",), shape)


# ================================================================================== 3. only the selected rows are read
@gpu
@pytest.mark.parametrize("shape", [po.SHAPES12[0], po.SHAPES12[2]])
def test_only_the_selected_rows_of_the_table_are_read(shape):
    """Per agent (a one-agent shard with its agent_offset): the own row and every row that is not a neighbour
    column of its sel overwritten with NaN gives the same bits."""
    _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    s = solver(N, Ko, Kn)
    table = np.array(R["table"])
    full = host_solve(s, R["b"], nbr_plan=table)
    for a in range(A):
        t = np.full_like(table, np.nan)
        keep = [i for i in full["sel"][a, Ko:] if i >= 0]
        assert a not in keep and len(keep) == Kn
        t[keep] = table[keep]
        one = host_solve(s, R["b"], slice(a, a + 1), nbr_plan=t, agent_offset=a)
        for k in OUT_KEYS + ("plan",):
            assert np.array_equal(one[k][0], full[k][a]), (a, k)


# ================================================================================== 4. curved tables: the certificate
@gpu
@pytest.mark.parametrize("shape", [po.SHAPES12[0], po.SHAPES12[1]])
def test_curved_tables_pass_the_kkt_certificate(shape):
    """The table is the plan output of a first device solve; every converged agent's point is a KKT point of the
    problem whose neighbour rows are the table's."""
    _need_gpu()
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    p, b = R["p"], R["b"]
    s = solver(N, Ko, Kn)
    first = host_solve(s, b)
    table = np.ascontiguousarray(first["plan"])
    assert np.abs(table - po.cv_table(p, b["nbr_state"])).max() > 1e-3       # not the constant-velocity lines
    out = host_solve(s, b, nbr_plan=table)
    ok = _opt(out["status"])
    assert ok.sum() >= _opt(first["status"]).sum() - 1, (out["status"].tolist(), first["status"].tolist())
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    for a in np.where(ok)[0]:
        cert = certified(p, b, a, table, out["sel"][a], out["x"][a])
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
    print(f"shape {shape}: {ok.sum()}/{A} converged (plain {_opt(first['status']).sum()}), worst certificate {worst}, "
          f"max |x - x(no table)| {np.abs(out['x'] - first['x']).max():.3e}")


# ================================================================================== 5. plan is the gather of x
@gpu
def test_plan_output_is_the_gather_of_x():
    torch = _need_gpu()
    shape = po.SHAPES12[0]
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    s = solver(N, Ko, Kn)
    table = np.array(R["table"])
    for kw in (dict(), dict(nbr_plan=table)):
        h = host_solve(s, R["b"], **kw)
        assert np.array_equal(h["plan"], po.plans_of(N, h["x"]))
        t = dev_batch(torch, R["b"])
        o = dev_out(torch, s, A, R["b"]["obstacles"].shape[0], A)
        d = dev_solve(torch, s, t, o, **{k: dev(torch, v) for k, v in kw.items()})
        assert np.array_equal(d["plan"], po.plans_of(N, d["x"]))
        assert_same(d, h, OUT_KEYS + ("plan",), "device entry vs host entry")
    # without out["plan"] nothing else changes
    o = dev_out(torch, s, A, R["b"]["obstacles"].shape[0], A, plan=False)
    assert_same(dev_solve(torch, s, dev_batch(torch, R["b"]), o, nbr_plan=dev(torch, table)), h, OUT_KEYS)


@gpu
def test_plan_output_of_the_qp_only_solve_with_a_rejected_polish():
    """use_nlp = 0: plan is written from the QP x, the table is ignored, and the agents whose polish was rejected
    (status 4) have their plans like everyone else."""
    _need_gpu()
    b, kw = _rejected_polish_batch()
    A, N = b["x0"].shape[0], 10
    s = solver(N, 3, 8, use_nlp=0, **kw)
    out = host_solve(s, b)
    assert (out["status"][:, 0] == 4).any() and np.isin(out["status"][:, 0], (0, 4)).all()
    assert np.array_equal(out["plan"], po.plans_of(N, out["x"]))
    nan = np.full((A, N, 2), np.nan)
    assert_same(host_solve(s, b, nbr_plan=nan), out, OUT_KEYS + ("plan",), "QP only: the table is never read")


# ================================================================================== 6. shards
@gpu
def test_shards_with_the_full_table_equal_the_full_batch():
    _need_gpu()
    shape = po.SHAPES12[0]
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    s = solver(N, Ko, Kn)
    table = np.array(R["table"])
    for sel in (False, True):
        full = host_solve(s, R["b"], nbr_plan=table, plan_selection=sel)
        for lo in range(0, A, A // 4):
            part = host_solve(s, R["b"], slice(lo, lo + A // 4), nbr_plan=table, agent_offset=lo, plan_selection=sel)
            for k in OUT_KEYS + ("plan",):
                assert np.array_equal(part[k], full[k][lo:lo + A // 4]), (k, lo, sel)


# ================================================================================== 7. horizon-aware selection
def crossing12(b, N, seed):
    """Crossing plans around the batch's own positions (as test_nbr_plan.crossing_tables: fast velocities and a
    curvature term, so agents that are distant now pass close later): plan [n][N][2], row k at Ts (k + 1)."""
    rng = np.random.default_rng(seed)
    pos = b["nbr_state"][:, :2]
    n = pos.shape[0]
    vel, acc = rng.normal(0, 12.0, (n, 2)), rng.normal(0, 40.0, (n, 2))
    t = workload.TS * np.arange(1, N + 1)
    return np.ascontiguousarray(pos[:, None] + vel[:, None] * t[None, :, None] + 0.5 * acc[:, None] * (t * t)[None, :, None])


def lip_rows(b):
    return np.ascontiguousarray(b["x0"][:, [0, 6, 1, 7]])


@gpu
@pytest.mark.parametrize("n_all", [3, 9, 40])
@pytest.mark.parametrize("Kn", [2, 8])
def test_horizon_aware_selection_against_brute_force(n_all, Kn):
    """The neighbour columns of sel with plan_selection against the numpy brute force of the header's definition;
    n_all = 3 with K_nbr = 8 has fewer agents than K_nbr (the columns clamp to the rows that exist).  The static
    columns are the snapshot selection's."""
    _need_gpu()
    N, Ko = 10, 2
    b = workload.make_batch12(n_all, N, "trot", seed=200 + n_all)
    plan = crossing12(b, N, 300 + n_all)
    s = solver(N, Ko, Kn)
    kn = min(Kn, n_all - 1)
    ref = brute_force(lip_rows(b), b["nbr_state"], plan, kn)
    snap = brute_force(lip_rows(b), b["nbr_state"], plan, kn, horizon=False)
    got = host_solve(s, b, nbr_plan=plan, plan_selection=True)["sel"]
    old = host_solve(s, b, nbr_plan=plan)["sel"]
    assert got.shape == (n_all, Ko + kn)
    assert np.array_equal(got[:, Ko:], ref), np.where((got[:, Ko:] != ref).any(1))[0]
    assert np.array_equal(old[:, Ko:], snap) and np.array_equal(got[:, :Ko], old[:, :Ko])
    if n_all == 40:
        differ = sum(set(ref[a]) != set(snap[a]) for a in range(n_all))
        assert differ >= 1, differ
    # a shard of the team
    if n_all == 40:
        part = host_solve(s, b, slice(13, 29), nbr_plan=plan, plan_selection=True, agent_offset=13)["sel"]
        assert np.array_equal(part, got[13:29])


def _moved(b, pos):
    """The batch with every agent moved to pos [A][2]: start, reference line and footholds shifted alike."""
    b = {k: np.array(v) for k, v in b.items()}
    d = pos - b["x0"][:, :2]
    b["x0"][:, :2] = pos
    b["xref"][:, :, :2] += d[:, None]
    b["foot"][:, :, :, :2] += d[:, None, None]
    b["nbr_state"][:, :2] = pos
    return b


@gpu
def test_horizon_aware_selection_ties_nan_rows_and_the_missing_columns():
    _need_gpu()
    N, Ko, Kn = 10, 1, 2
    s = solver(N, Ko, Kn)
    # exactly representable coordinates (tests/test_nbr_plan.py): agent 0 rests at the origin, rows 1 and 2 rest at
    # distance 5 on opposite sides (an exact tie: the lower index wins), row 3 starts far away and passes at
    # distance 1 at grid 4, row 4 is nearest now (distance 4) and leaves.
    n_all = 6
    pos = np.array([[0.0, 0.0], [3.0, 4.0], [-3.0, -4.0], [64.0, 1.0], [0.0, 4.0], [100.0, 100.0]])
    b = _moved(workload.make_batch12(n_all, N, "stand", seed=7), pos)
    b["obstacles"] = np.array([[50.0, 50.0]])
    b["x0"][:, 6:8] = 0.0; b["nbr_state"][:, 2:] = 0.0
    plan = np.ascontiguousarray(np.repeat(pos[:, None], N, 1))
    plan[3, :, 0] = 64.0 - 16.0 * np.arange(1, N + 1)
    plan[4, :, 1] = 4.0 + 8.0 * np.arange(1, N + 1)
    ref = brute_force(lip_rows(b), b["nbr_state"], plan, Kn)
    assert ref[0].tolist() == [3, 4]
    got = host_solve(s, b, nbr_plan=plan, plan_selection=True)["sel"]
    assert np.array_equal(got[:, Ko:], ref)
    far = plan.copy(); far[3] += 1000.0; far[4] += 1000.0
    pos2 = pos.copy(); pos2[3] += 1000.0; pos2[4] += 1000.0
    b2 = _moved(b, pos2)
    ref2 = brute_force(lip_rows(b2), b2["nbr_state"], far, Kn)
    assert ref2[0].tolist() == [1, 2]
    got2 = host_solve(s, b2, nbr_plan=far, plan_selection=True)["sel"]
    assert np.array_equal(got2[:, Ko:], ref2)
    # rows with a NaN anywhere in their plan or snapshot are never selected: fewer than Kn rows remain -> -1
    b4 = workload.make_batch12(4, N, "trot", seed=9)
    plan4 = crossing12(b4, N, 9)
    plan4[1, 7, 1] = np.nan
    b4["nbr_state"] = np.array(b4["nbr_state"]); b4["nbr_state"][2, 0] = np.nan
    ref4 = brute_force(lip_rows(b4), b4["nbr_state"], plan4, Kn)
    assert ref4[0].tolist() == [3, -1] and ref4[3].tolist() == [0, -1]
    out4 = host_solve(s, b4, nbr_plan=plan4, plan_selection=True)
    assert np.array_equal(out4["sel"][:, Ko:], ref4)


@gpu
def test_horizon_aware_selection_scans_the_agents_scene_only():
    _need_gpu()
    S, team, n_obs, N, Ko, Kn = 3, 4, 5, 10, 2, 2
    b = workload.make_scenes12(S, team, N, "trot", seed=23, n_obs=n_obs)
    plan = crossing12(b, N, 24)
    s = solver(N, Ko, Kn)
    s.set_scenes(team, n_obs)
    try:
        got = host_solve(s, b, nbr_plan=plan, plan_selection=True)["sel"]
        old = host_solve(s, b, nbr_plan=plan)["sel"]
    finally:
        s.set_scenes(0, 0)
    kn = min(Kn, team - 1)
    assert got.shape == (S * team, Ko + kn)
    x0 = lip_rows(b)
    differ = 0
    for i in range(S):
        r = slice(i * team, (i + 1) * team)
        ref = brute_force(x0[r], b["nbr_state"][r], plan[r], kn)
        snap = brute_force(x0[r], b["nbr_state"][r], plan[r], kn, horizon=False)
        assert np.array_equal(got[r, Ko:], ref + i * team), i
        assert np.array_equal(old[r, Ko:], snap + i * team), i
        differ += int((ref != snap).any())
    assert differ >= 1                                       # (numpy alone: all three scenes of this draw differ)


# ================================================================================== 8. the shift kernel
@gpu
@pytest.mark.parametrize("N,grids", [(4, 4), (5, 4), (10, 4), (10, 0), (10, 13), (2, 1)])
def test_shift_kernel_equals_dist_shift_plans(N, grids):
    """N = 4 with grids 4 keeps nothing; A = 300 is more than one block with a partial last one, and an agent's
    grids straddle blocks."""
    torch = _need_gpu()
    A = 300
    s = solver(N, 1, 0, max_agents=320)
    plan = np.random.default_rng(N + grids).normal(size=(A, N, 2))
    plan[5, N - 1, 0] = np.nan
    want = sdist.shift_plans(torch.as_tensor(plan), grids).numpy()
    assert np.array_equal(want, po.shift(plan, grids), equal_nan=True)
    table = torch.full((A + 1, N, 2), -7.0, dtype=torch.float64, device="cuda")
    s.shift_plans_device(dev(torch, plan), table[:A], grids)
    torch.cuda.synchronize()
    assert np.array_equal(table[:A].cpu().numpy(), want, equal_nan=True)
    assert (table[A] == -7.0).all()                          # nothing past the last agent


# ================================================================================== 9. the coupled driver
@gpu
def test_coupled_driver_equals_manual_rounds():
    torch = _need_gpu()
    shape = po.SHAPES12[0]
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    s = solver(N, Ko, Kn)
    t = dev_batch(torch, R["b"])
    n_obs = R["b"]["obstacles"].shape[0]
    rounds, table = [], None
    for r in range(3):
        o = dev_out(torch, s, A, n_obs, A)
        rounds.append(dev_solve(torch, s, t, o, nbr_plan=table))
        table = o["plan"]
    o = dev_out(torch, s, A, n_obs, A)
    change = s.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o, outer=3)
    torch.cuda.synchronize()
    assert_same(host(o), rounds[2], OUT_KEYS + ("plan",), "outer = 3")
    want = [np.abs(rounds[r]["plan"] - rounds[r - 1]["plan"]).max() for r in (1, 2)]
    assert change.shape == (2,) and change.is_cuda and change.cpu().tolist() == want
    print(f"plan_change per Jacobi round: {want}")
    assert want[0] > 1e-6                                      # the iteration moves the plans at all
    o1 = dev_out(torch, s, A, n_obs, A)
    c1 = s.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o1, outer=1)
    torch.cuda.synchronize()
    assert c1.numel() == 0
    assert_same(host(o1), rounds[0], OUT_KEYS + ("plan",), "outer = 1")
    # a one-rank dist.PlanExchange-shaped exchange (a callable on the plan tensor) is used as it is
    calls = []

    def exchange(plan):
        calls.append(plan.data_ptr())
        return plan.clone()
    o2 = dev_out(torch, s, A, n_obs, A)
    s.solve_coupled_device(t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"], t["nbr_state"], o2, outer=3,
                           exchange=exchange)
    torch.cuda.synchronize()
    assert len(calls) == 2 and calls[0] != calls[1]
    assert_same(host(o2), rounds[2], OUT_KEYS + ("plan",), "with an exchange")


# ================================================================================== 10. the rollout with plans
ROLLS = [(12, 10, "trot", 5, 5, 3, 4), (8, 6, "stand", 7, 5, 1, 2)]      # (A, N, gait, seed, T, K_obs, K_nbr)
_rolls = {}


def roll12(run, plans, mode):
    """One of ROLLS on the device with log_x, once per (run, plans, mode): the host copies of results()."""
    key = (run, plans, mode)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, gait, seed, T, Ko, Kn = run
        state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
        r = srb12.Rollout12(solver(N, Ko, Kn), dev(torch, goal), phase=dev(torch, phase), gait=gait, log_x=True,
                            obstacles=dev(torch, obstacles), plans=plans)
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
@pytest.mark.parametrize("run", ROLLS)
def test_rollout_c_driver_equals_python_steps_bitwise(run):
    for plans in (True, False):
        a, b = roll12(run, plans, "run"), roll12(run, plans, "step")
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), (plans, k)
    on, off = roll12(run, True, "run"), roll12(run, False, "run")
    # the first cycle has no table: the plans-off rollout's bits
    for k in ("x", "status", "iters"):
        assert np.array_equal(on[k][0], off[k][0]), k
    assert np.array_equal(on["traj"][:2], off["traj"][:2])
    assert not np.array_equal(on["x"][1:], off["x"][1:])      # later cycles read the table


@gpu
@pytest.mark.parametrize("run", ROLLS)
def test_rollout_every_cycle_is_the_solve_against_the_shifted_previous_plans(run):
    """Every later cycle's logged x is, bitwise, a stand-alone solve_device on that cycle's inputs (the advance of
    the logged state, with the cycle index folded into the phase) against the table rebuilt from the previous
    logged x by the numpy shift; two agents a cycle pass the KKT certificate with the table's rows; the safety
    metrics are sim_oracle's restatement on the logged trajectory."""
    torch = _need_gpu()
    A, N, gait, seed, T, Ko, Kn = run
    res = roll12(run, True, "run")
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, seed)
    s = solver(N, Ko, Kn)
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    assert res["cycles"] == T and res["x"].shape == (T, A, 24 * N + 1)
    n_cert = 0
    for c in range(T):
        assert np.array_equal(res["traj"][c + 1], res["x"][c][:, 36:48]), c
        r = srb12.Rollout12(s, dev(torch, goal), phase=dev(torch, (phase + c).astype(np.int32)), gait=gait,
                            obstacles=dev(torch, obstacles))
        r.reset(dev(torch, res["traj"][c]))
        r.advance()
        table = None if c == 0 else po.shift(po.plans_of(N, res["x"][c - 1]), 4)
        o = dev_out(torch, s, A, obstacles.shape[0], A)
        s.solve_device(r.x0, r.xref, r.foot, r.contact, r.obstacles, r.last_state, o,
                       nbr_plan=None if table is None else dev(torch, table))
        torch.cuda.synchronize()
        got = host(o)
        assert np.array_equal(got["x"], res["x"][c]), c
        assert np.array_equal(got["status"], res["status"][c]) and np.array_equal(got["iters"], res["iters"][c]), c
        if c == 0:
            continue
        b = dict(x0=r.x0.cpu().numpy(), xref=r.xref.cpu().numpy(), foot=r.foot.cpu().numpy(),
                 contact=r.contact.cpu().numpy(), obstacles=obstacles, nbr_state=r.last_state.cpu().numpy())
        for a in np.where(_opt(got["status"]))[0][:2]:
            certified(p, b, a, table, got["sel"][a], got["x"][a])
            n_cert += 1
    assert n_cert >= 2 * (T - 1) - 2
    m = sim_oracle.Metrics(0)
    for c in range(T):
        st = res["traj"][c]
        m.update(c, sim12_oracle.com_of(st), obstacles, st[:, [0, 1, 6, 7]])
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), (k, res[k], v)


# ================================================================================== 11. scenes with plans
@gpu
def test_scenes_with_plans_equal_the_per_team_runs_bitwise():
    torch = _need_gpu()
    S, team, n_obs, N, Ko, Kn, T = 4, 4, 5, 10, 3, 8, 3
    b = workload.make_scenes12(S, team, N, "trot", seed=31, n_obs=n_obs)
    s = solver(N, Ko, Kn)
    table = po.plans_of(N, host_solve(s, b)["x"])            # some curved table, scene-major like the snapshot

    def team_solve(i, **kw):
        r, ob = slice(i * team, (i + 1) * team), slice(i * n_obs, (i + 1) * n_obs)
        return s.solve(b["x0"][r], b["xref"][r], b["foot"][r], b["contact"][r], b["obstacles"][ob], b["nbr_state"][r],
                       nbr_plan=np.ascontiguousarray(table[r]), **kw)

    def team_roll(rows, obs):
        r = srb12.Rollout12(s, dev(torch, b["goal"][rows]), phase=dev(torch, b["phase"][rows]), log_x=True,
                            obstacles=dev(torch, b["obstacles"][obs]), plans=True, plan_selection=True)
        r.reset(dev(torch, b["x0"][rows]))
        r.run(T)
        res = r.results()
        torch.cuda.synchronize()
        return host(res)
    for sel in (False, True):
        teams = [team_solve(i, plan_selection=sel) for i in range(S)]
        s.set_scenes(team, n_obs)
        try:
            out = host_solve(s, b, nbr_plan=table, plan_selection=sel)
        finally:
            s.set_scenes(0, 0)
        for i, t in enumerate(teams):
            r = slice(i * team, (i + 1) * team)
            for k in ("x", "x_qp", "status", "iters", "obj", "plan"):
                assert np.array_equal(out[k][r], t[k]), (sel, i, k)
            want = t["sel"].copy()
            want[:, :Ko] = np.where(want[:, :Ko] >= 0, want[:, :Ko] + i * n_obs, want[:, :Ko])
            want[:, Ko:] = np.where(want[:, Ko:] >= 0, want[:, Ko:] + i * team, want[:, Ko:])
            assert np.array_equal(out["sel"][r], want), (sel, i)
    teams = [team_roll(slice(i * team, (i + 1) * team), slice(i * n_obs, (i + 1) * n_obs)) for i in range(S)]
    s.set_scenes(team, n_obs)
    try:
        got = team_roll(slice(None), slice(None))
    finally:
        s.set_scenes(0, 0)
    for k, v in got.items():
        if k == "cycles":
            assert v == T
            continue
        cat = np.concatenate([t[k] for t in teams], 1 if v.ndim > 1 and k != "state" else 0)
        assert np.array_equal(v, cat), k


# ================================================================================== 12. refusals with a live context
@gpu
def test_refusals_by_name_and_the_context_survives():
    torch = _need_gpu()
    shape = po.SHAPES12[0]
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    b = R["b"]
    s = solver(N, Ko, Kn)
    table = np.array(R["table"])
    good = host_solve(s, b, nbr_plan=table)
    t = dev_batch(torch, b)
    n_obs = b["obstacles"].shape[0]
    o = dev_out(torch, s, A, n_obs, A)
    dt = dev(torch, table)

    def refused(msg, fn):
        with pytest.raises(RuntimeError, match=msg) as e:
            fn()
        assert "srbnmpc error -1:" in str(e.value)              # SRB_ERR_ARG
        again = host_solve(s, b, nbr_plan=table)                # a following valid solve succeeds
        assert np.array_equal(again["x"], good["x"]) and np.array_equal(again["status"], good["status"])
    args = (t["x0"], t["xref"], t["foot"], t["contact"], t["obstacles"])
    refused("nbr_plan needs nbr_state",
            lambda: s.solve(b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], None, nbr_plan=table))
    no_sel = {k: v for k, v in o.items() if k != "sel"}        # (without the snapshot sel would be [A][K_obs])
    refused("nbr_plan needs nbr_state", lambda: s.solve_device(*args, None, no_sel, nbr_plan=dt))
    refused("agent_offset", lambda: s.solve_device(*args, t["nbr_state"], o, nbr_plan=dt, agent_offset=1))
    refused("agent_offset", lambda: host_solve(s, b, nbr_plan=table, agent_offset=1))
    refused("plan_selection = 1 needs nbr_plan", lambda: s.solve_device(*args, t["nbr_state"], o, plan_selection=True))
    refused("plan_selection = 1 needs nbr_plan", lambda: host_solve(s, b, plan_selection=True))
    refused("plan overlaps the nbr_plan table", lambda: s.solve_device(*args, t["nbr_state"], o, nbr_plan=dt, plan=dt))
    big = torch.zeros(2 * A - 1, N, 2, dtype=torch.float64, device="cuda")
    refused("plan overlaps", lambda: s.solve_device(*args, t["nbr_state"], o, nbr_plan=big[:A], plan=big[A - 1:]))
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    dp = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    st = s._stream(None)
    pl = srb12.Plans12(dp(dt), dp(o["plan"]), 0, None); pl.struct_size -= 8
    bat = srb12.Batch12()
    assert lib.srb12_solve_batch_plans_device(s._h, A, ctypes.byref(bat), ctypes.byref(pl), st) == -1
    assert "srb12_plans.struct_size" in err()
    assert lib.srb12_shift_plans_device(s._h, A, dp(dt), -1, dp(o["plan"]), st) == -1 and "grids must be >= 0" in err()
    assert lib.srb12_shift_plans_device(s._h, A, dp(dt), 4, dp(dt), st) == -1 and "two buffers" in err()
    assert lib.srb12_shift_plans_device(s._h, A, dp(big), 4, dp(big[1:]), st) == -1 and "overlap" in err()
    assert lib.srb12_shift_plans_device(s._h, 65, dp(dt), 4, dp(o["plan"]), st) == -1 and "max_agents" in err()
    s1 = srb12.Solver12(srb12.default_params(1, K_obs=1, K_nbr=0), 4)
    assert lib.srb12_shift_plans_device(s1._h, 4, dp(dt), 4, dp(o["plan"]), s1._stream(None)) == -1 and "N >= 2" in err()
    s1.close()
    # the rollout driver: a shard, and plan == plan_table
    state, goal, obstacles, phase = sim12_oracle.team12(A, N, gait, 5)
    r = srb12.Rollout12(s, dev(torch, goal), obstacles=dev(torch, obstacles), plans=True)
    r.reset(dev(torch, state))
    r._reserve(2)
    ro = r.out
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)

    def call(plans, **kw):
        bb = srb12.Batch12(None, None, None, None, dp(r.obstacles), None, r.obstacles.shape[0], A, 0, None, dp(ro["x"]),
                           dp(ro["obj"]), ip(ro["status"]), ip(ro["iters"]), None, 0)
        for k, v in kw.items():
            setattr(bb, k, v)
        return lib.srb12_rollout_plans_device(s._h, A, ctypes.byref(bb), ctypes.byref(r._sim()), ctypes.byref(plans), 1, st)
    assert call(srb12.Plans12(None, dp(ro["plan"]), 0, dp(r.plan_table)), agent_offset=1) == -1 and "sharded" in err()
    assert call(srb12.Plans12(None, dp(ro["plan"]), 0, dp(ro["plan"]))) == -1 and "plan overlaps plan_table" in err()
    assert call(srb12.Plans12(None, None, 0, dp(r.plan_table))) == -1 and "needs srb12_plans.plan" in err()
    with pytest.raises(ValueError, match="plan_selection needs plans=True"):
        srb12.Rollout12(s, dev(torch, goal), plan_selection=True)
    # after the refusals the same objects work as if nothing had happened
    r.run(2)
    res = r.results()
    torch.cuda.synchronize()
    assert res["cycles"] == 2 and res["status"].shape == (2, A, 2)
    again = dev_solve(torch, s, t, o, nbr_plan=dt)
    assert_same(again, good, OUT_KEYS + ("plan",), "after the refusals")
