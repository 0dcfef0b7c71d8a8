"""Obstacle sizes: srb_sizes (obs_eps, obs_radius, clearance_selection) through the selection, the solve, the metrics
and the rollout.

The reference is tests/sizes_oracle.py: the oracle's own chain per agent with the levels of its static columns taken
from the table, and numpy restatements of the clearance selection and of the sized metrics.  Tolerances are the
project's (test_moving_obstacles.assert_matches): statuses equal; X, U, s within 1e-4 (the full x too at C = 2); obj at
rtol 1e-7 / atol 1e-6; iterations equal on at least 85 % of the agents and never off by more than 2.  Selections,
metrics, "off is off", run == steps, shards and scenes are compared bit for bit.  The shapes are plan_oracle.SHAPES
and the closed-loop runs moving_oracle.RUNS; the table is workload.obstacle_sizes (eps ~ U[0.6, 3.6]).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import moving_oracle
import oracle
import plan_oracle
import sim_oracle
import sizes_oracle
import srbnmpc
import test_moving_obstacles as tmo
from srbnmpc import dist as sdist
from srbnmpc import workload

SHAPES = plan_oracle.SHAPES
SHAPE_C2 = SHAPES[1]
RUNS = moving_oracle.RUNS
# the conditions that make the GPU tests mean something: half of what the oracle measured for the drawn table
MOVED_MIN = dict(zip(SHAPES, (4, 24, 6, 5)))          # agents the table moves by > 1e-3 (measured 7 / 49 / 13 / 10)
DIFFER_MIN = dict(zip(SHAPES, (1, 29, 6, 1)))         # agents whose clearance selection differs (measured 3 / 58 / 12 / 3)
OUT_KEYS = tmo.OUT_KEYS
NEW_SYMBOLS = ("srb_solve_batch_sized", "srb_solve_batch_sized_device", "srb_select_sized_device",
               "srb_sim_metrics_sized_device", "srb_rollout_sized_device")
gpu = pytest.mark.gpu
_dp = ctypes.POINTER(ctypes.c_double)
EPS_OBS = float(np.float32(1.9))
assert_matches, xus, solver, dev, host, host_solve, device_solve = (tmo.assert_matches, tmo.xus, tmo.solver, tmo.dev,
                                                                    tmo.host, tmo.host_solve, tmo.device_solve)


# ============================================================================================ CPU
def test_sizes_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(srb_sizes), offsetof(srb_sizes, struct_size), '
                   'offsetof(srb_sizes, obs_eps), offsetof(srb_sizes, obs_radius), offsetof(srb_sizes, clearance_selection));'
                   ' return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = srbnmpc.Sizes
    assert got == [ctypes.sizeof(S), S.struct_size.offset, S.obs_eps.offset, S.obs_radius.offset,
                   S.clearance_selection.offset]
    assert srbnmpc.Sizes().struct_size == ctypes.sizeof(S)


def test_abi_version_is_still_6_and_the_old_layouts_stand():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert srbnmpc.lib().srb_abi_version() == 6 and srbnmpc.ABI_VERSION == 6
    assert srbnmpc.Batch._fields_[-1][0] == "plan" and srbnmpc.Sim._fields_[-1][0] == "distance_to_fail"
    assert [f[0] for f in srbnmpc.Moving._fields_] == ["struct_size", "obs_vel", "horizon_selection", "obstacles"]


def test_every_new_symbol_is_exported():
    L = srbnmpc.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name


def test_obstacle_sizes_are_deterministic_in_range_and_leave_the_other_draws_alone():
    before = (workload.make_batch(8, 10, 2, seed=5), workload.obstacle_velocities(20, 5),
              workload.make_scenes(2, 4, 10, 2, seed=5, n_obs=5))
    for n, seed in ((20, 5), (320, 12), (1, 0)):
        eps, rad = workload.obstacle_sizes(n, seed)
        for v in (eps, rad):
            assert v.shape == (n,) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"]
        e2, r2 = workload.obstacle_sizes(n, seed)
        assert np.array_equal(eps, e2) and np.array_equal(rad, r2)
        assert (eps >= 0.6).all() and (eps <= 3.6).all()
        assert np.array_equal(eps, np.random.default_rng(200 + seed).uniform(0.6, 3.6, n))
        assert np.array_equal(rad, 0.5 * np.sqrt(eps / EPS_OBS))
    assert not np.array_equal(workload.obstacle_sizes(20, 5)[0], workload.obstacle_sizes(20, 6)[0])
    # eps_obs itself gives the reference's fail radius
    assert 0.5 * np.sqrt(EPS_OBS / EPS_OBS) == 0.5 and workload.EPS_OBS == EPS_OBS
    after = (workload.make_batch(8, 10, 2, seed=5), workload.obstacle_velocities(20, 5),
             workload.make_scenes(2, 4, 10, 2, seed=5, n_obs=5))
    assert np.array_equal(before[1], after[1])
    for a, b in ((before[0], after[0]), (before[2], after[2])):
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k


def test_python_layer_validates_the_tables_by_name():
    chk = srbnmpc._check_size_array
    for name in ("obs_eps", "obs_radius"):
        with pytest.raises(ValueError, match=name):
            chk(np.zeros(4, np.float32), 4, np.float64, name)
        with pytest.raises(ValueError, match=name):
            chk(np.zeros(5), 4, np.float64, name)
        with pytest.raises(ValueError, match=name):
            chk(np.zeros((4, 1)), 4, np.float64, name)
        with pytest.raises(ValueError, match=name):
            chk(np.zeros(8)[::2], 4, np.float64, name)
        with pytest.raises(ValueError, match=name):
            chk([1.0] * 4, 4, np.float64, name)
        chk(np.zeros(4), 4, np.float64, name)


def _refusal_cases():
    """(entry, sizes, word) of every refusal of srb_sizes; none needs a context: the checks run before the context
    is looked at, so a null context reaches them (with a live context nothing is launched either: the GPU test)."""
    eps = np.ones(3)
    pe = eps.ctypes.data_as(_dp)
    S = srbnmpc.Sizes
    bad_size = S(pe, None, 0)
    bad_size.struct_size += 8
    cases = []
    for entry in ("solve", "select", "metrics", "rollout"):
        cases += [(entry, bad_size, "srb_sizes.struct_size"), (entry, S(pe, None, 2), "srb_sizes.clearance_selection"),
                  (entry, S(pe, None, -1), "srb_sizes.clearance_selection"),
                  (entry, S(None, pe, 1), "clearance_selection = 1 needs obs_eps")]
    return (eps,), cases


def _call_refused(lib, h, entry, sz, b=None, n_agents=1):
    b = srbnmpc.Batch() if b is None else b
    sim = srbnmpc.Sim()
    if entry == "rollout":
        return lib.srb_rollout_sized_device(h, n_agents, ctypes.byref(b), ctypes.byref(sim), None, ctypes.byref(sz), 1, None)
    if entry == "metrics":
        return lib.srb_sim_metrics_sized_device(h, n_agents, ctypes.byref(sim), ctypes.byref(sz), 0, None)
    if entry == "select":
        return lib.srb_select_sized_device(h, n_agents, ctypes.byref(b), None, ctypes.byref(sz), 1, None)
    rcs = {lib.srb_solve_batch_sized(h, n_agents, ctypes.byref(b), None, ctypes.byref(sz)),
           lib.srb_solve_batch_sized_device(h, n_agents, ctypes.byref(b), None, ctypes.byref(sz), None)}
    assert len(rcs) == 1, rcs
    return rcs.pop()


def test_refusals_by_name_without_a_context():
    lib = srbnmpc.lib()
    keep, cases = _refusal_cases()
    for entry, sz, word in cases:
        assert _call_refused(lib, None, entry, sz) == -1, (entry, word)
        assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())
    # obs_eps beside a versioned table is no refusal of srb_sizes: the call gets as far as the missing context
    b = srbnmpc.Batch()
    b.obstacles_version = 7
    assert _call_refused(lib, None, "solve", srbnmpc.Sizes(keep[0].ctypes.data_as(_dp), None, 0), b) == -1
    assert "null argument" in lib.srb_last_error().decode()
    # ... and the srb_moving refusals are still made by these entry points
    mv = srbnmpc.Moving(None, 1, None)
    assert lib.srb_solve_batch_sized(None, 1, ctypes.byref(b), ctypes.byref(mv), None) == -1
    assert "horizon_selection = 1 needs obs_vel" in lib.srb_last_error().decode()


@pytest.mark.parametrize("shape", SHAPES)
def test_helper_with_a_uniform_table_equals_oracle_batch(shape):
    R = plan_oracle.reference(shape)
    r = sizes_oracle.solve(R["p"], R["b"], np.full(R["b"]["obstacles"].shape[0], EPS_OBS))
    assert R["p"].eps_obs == EPS_OBS
    for k in ("x_qp", "x", "status", "iters"):
        assert np.array_equal(r[k], R["r0"][k]), k


def moved_agents(shape, key="r"):
    R = sizes_oracle.reference(shape)
    N = shape[0]
    return int((np.abs(R[key]["x"][:, :6 * N] - R["r0"]["x"][:, :6 * N]).max(1) > 1e-3).sum())


@pytest.mark.parametrize("shape", SHAPES)
def test_the_drawn_table_matters_and_every_solve_is_optimal(shape):
    R = sizes_oracle.reference(shape)
    Ko = shape[2]
    for key in ("r", "rc"):
        assert (R[key]["status"][:, 1] == 0).all() and np.isin(R[key]["status"][:, 0], (0, 4)).all(), key
    differ = int((R["sel_c"][:, :Ko] != R["r"]["sel"][:, :Ko]).any(1).sum())
    keys = sizes_oracle.clearance_keys(R["b"]["x0"], R["b"]["obstacles"], R["eps"])
    print(f"{shape}: moved {moved_agents(shape)} (centres) / {moved_agents(shape, 'rc')} (clearance), selection differs "
          f"for {differ}, {int((keys < 0).sum())} negative keys")
    assert moved_agents(shape) >= MOVED_MIN[shape], moved_agents(shape)
    assert differ >= DIFFER_MIN[shape], differ
    assert (keys < 0).any()                              # agents start inside a level set: negative keys are exercised


# smallest / median of the closed loop's min_d_obs (clearance to the bodies, m), static and moving world, as printed
CLOSED_LOOP_PINS = {False: (-0.1115, 0.3213), True: (-0.3107, 0.2480)}


def test_oracle_closed_loop_with_sizes():
    """moving_oracle.RUNS[2] with the drawn sizes, oracle only, static and moving: every NLP status OPTIMAL; the
    smallest and median minimum clearance it prints, pinned at the 6e-4 of the moving test."""
    run = RUNS[2]
    for moving, (lo, med) in CLOSED_LOOP_PINS.items():
        L = sizes_oracle.closed_loop(run, moving)
        assert (L["status"][..., 1] == 0).all() and np.isin(L["status"][..., 0], (0, 4)).all()
        d = L["metrics"]["min_d_obs"]
        print(f"moving={moving}: min_d_obs smallest {d.min():.4f} median {np.median(d):.4f}, "
              f"{int((L['metrics']['fail_cycle'] >= 0).sum())} agents cross a body radius")
        assert abs(d.min() - lo) < 6e-4 and abs(np.median(d) - med) < 6e-4


# ============================================================================================ GPU
_need_gpu = tmo._need_gpu


# ---------------------------------------------------------------------------- 1. off is off
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_no_table_and_a_uniform_table_give_the_bits_of_the_plain_call(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, seed = shape
    b = plan_oracle.reference(shape)["b"]
    n_obs = b["obstacles"].shape[0]
    s = solver(N, C, Ko, Kn)
    uni = np.full(n_obs, EPS_OBS)
    plain, dplain = host_solve(s, b), device_solve(torch, s, b)
    lib = srbnmpc.lib()

    def raw_host(mv, sz):
        """srb_solve_batch_sized itself, so that sz == NULL and an all-NULL sz are reached."""
        out = host_solve(s, b)                                 # buffers of the right shapes, then overwritten
        for v in out.values():
            v.fill(0)
        x0, ref, foot = (np.ascontiguousarray(b[k], dtype=np.float64) for k in ("x0", "ref", "foot"))
        ob, nb = np.ascontiguousarray(b["obstacles"]), np.ascontiguousarray(b["nbr_state"])
        P = srbnmpc._p
        bt = srbnmpc.Batch(P(x0), P(ref), P(foot), P(ob), P(nb), n_obs, nb.shape[0], 0, P(out["x_qp"]), P(out["x"]),
                           P(out["obj"]), P(out["status"]), P(out["iters"]), None, None, P(out["sel"]), 0, None, P(out["plan"]))
        srbnmpc._check(lib.srb_solve_batch_sized(s._h, A, ctypes.byref(bt), None if mv is None else ctypes.byref(mv),
                                                 None if sz is None else ctypes.byref(sz)))
        return out
    zero = np.zeros_like(b["obstacles"])
    vel = workload.obstacle_velocities(n_obs, seed)
    moving = host_solve(s, b, obs_vel=vel)
    cases = [("no sz", raw_host(None, None), plain), ("all-NULL sz", raw_host(None, srbnmpc.Sizes(None, None, 0)), plain),
             ("uniform", host_solve(s, b, obs_eps=uni), plain),
             ("uniform + zero vel", host_solve(s, b, obs_eps=uni, obs_vel=zero), plain),
             ("uniform + vel", host_solve(s, b, obs_eps=uni, obs_vel=vel), moving),
             ("all-NULL sz + vel", raw_host(srbnmpc.Moving(srbnmpc._p(vel), 0, None), srbnmpc.Sizes(None, None, 0)), moving),
             ("device uniform", device_solve(torch, s, b, obs_eps=uni), dplain),
             ("device uniform + zero vel", device_solve(torch, s, b, obs_eps=uni, obs_vel=zero), dplain),
             ("device uniform + vel", device_solve(torch, s, b, obs_eps=uni, obs_vel=vel), moving),
             ("host / device", dplain, plain)]
    for what, got, want in cases:
        for k in OUT_KEYS:
            assert np.array_equal(got[k], want[k]), (what, k)


# ---------------------------------------------------------------------------- 2. against the oracle
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_drawn_table_against_the_oracle(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = sizes_oracle.reference(shape)
    s = solver(N, C, Ko, Kn)
    eps = np.array(R["eps"])
    out = host_solve(s, R["b"], obs_eps=eps)
    assert_matches(N, C, out, R["r"], f"{shape} host")
    assert np.array_equal(out["sel"], R["r"]["sel"])
    d = device_solve(torch, s, R["b"], obs_eps=eps)
    for k in OUT_KEYS:
        assert np.array_equal(d[k], out[k]), k


@gpu
def test_drawn_table_with_a_velocity_table_and_with_neighbour_plans_against_the_oracle():
    torch = _need_gpu()
    N, C, Ko, Kn, A, seed = SHAPE_C2
    R = sizes_oracle.reference(SHAPE_C2)
    eps, b, p = np.array(R["eps"]), R["b"], R["p"]
    s = solver(N, C, Ko, Kn)
    vel = np.array(moving_oracle.reference(SHAPE_C2)["vel"])
    r = sizes_oracle.solve(p, b, eps, vel)
    out = host_solve(s, b, obs_eps=eps, obs_vel=vel)
    assert_matches(N, C, out, r, "sizes + velocities")
    assert np.array_equal(out["sel"], r["sel"])
    d = device_solve(torch, s, b, obs_eps=eps, obs_vel=vel)
    for k in OUT_KEYS:
        assert np.array_equal(d[k], out[k]), k
    # both tables matter: neither the sizes-only nor the velocity-only answer
    for other in (R["r"], moving_oracle.reference(SHAPE_C2)["r"]):
        assert (np.abs(xus(N, out["x"]) - xus(N, other["x"])).max(1) > 1e-3).sum() >= 4
    table = np.array(plan_oracle.reference(SHAPE_C2)["table"])
    rp = sizes_oracle.solve(p, b, eps, table=table)
    outp = host_solve(s, b, obs_eps=eps, nbr_plan=table)
    assert_matches(N, C, outp, rp, "sizes + plans")
    for other in (R["r"], plan_oracle.reference(SHAPE_C2)["r1"]):
        assert (np.abs(xus(N, outp["x"]) - xus(N, other["x"])).max(1) > 1e-3).sum() >= 4


# ---------------------------------------------------------------------------- 3. read only through sel
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_the_level_table_is_read_only_through_sel(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = sizes_oracle.reference(shape)
    s = solver(N, C, Ko, Kn)
    eps = np.array(R["eps"])
    good = host_solve(s, R["b"], obs_eps=eps)
    used = np.unique(good["sel"][:, :min(Ko, eps.shape[0])])
    assert used.size < eps.shape[0]
    holes = eps.copy()
    holes[np.setdiff1d(np.arange(eps.shape[0]), used)] = np.nan
    for out in (host_solve(s, R["b"], obs_eps=holes), device_solve(torch, s, R["b"], obs_eps=holes)):
        for k in OUT_KEYS:
            assert np.array_equal(out[k], good[k]), k


# ---------------------------------------------------------------------------- 4. clearance selection
WAVES = tmo.WAVES


def select(torch, s, x0, ob, nbr, eps=None, clear=False, vel=None, horizon=False, tables=3, agent_offset=0):
    Ko, Kn = s.n_selected(ob.shape[0], 0 if nbr is None else nbr.shape[0])
    sel = torch.full((x0.shape[0], Ko + Kn), -7, dtype=torch.int32, device="cuda")
    s.select_device(dev(torch, x0), dev(torch, ob), None if nbr is None else dev(torch, nbr), sel, tables=tables,
                    agent_offset=agent_offset, obs_vel=None if vel is None else dev(torch, vel), obs_horizon=horizon,
                    obs_eps=None if eps is None else dev(torch, eps), obs_clearance=clear)
    torch.cuda.synchronize()
    return sel.cpu().numpy()


@gpu
@pytest.mark.parametrize("horizon", [False, True])
@pytest.mark.parametrize("n_obs", [1, 3, 63, 64, 65, 64 * WAVES - 1, 64 * WAVES, 64 * WAVES + 1])
@pytest.mark.parametrize("Ko", [1, 3, 8])
def test_clearance_selection_index_for_index(n_obs, Ko, horizon):
    """Every row count either side of a lane, a wave and a scan pass (64 x the kernel's wave count); K_obs 1, 3, 8,
    and K_obs > n_obs (n_obs 1 and 3), which clamps to the rows that exist; the distance now and the horizon's."""
    torch = _need_gpu()
    N, A, Kn = 10, 9, 2
    s = solver(N, 2, Ko, Kn)
    x0, nbr, ob, vel = tmo.crossing_world(n_obs, A, 1000 * Ko + n_obs)
    eps = np.random.default_rng(7000 + 10 * n_obs + Ko).uniform(0.6, 3.6, n_obs)
    w = vel if horizon else None
    want = sizes_oracle.clearance_select(x0, ob, eps, Ko, s.params.Ts, N, w)
    got = select(torch, s, x0, ob, nbr, eps, True, w, horizon)
    ko = min(Ko, n_obs)
    assert got.shape == (A, ko + Kn) and want.shape == (A, ko)
    assert np.array_equal(got[:, :ko], want), np.where((got[:, :ko] != want).any(1))[0]
    # a velocity table without horizon_selection leaves the key at the distance now
    if not horizon:
        assert np.array_equal(select(torch, s, x0, ob, nbr, eps, True, vel, False)[:, :ko], want)
    # the neighbour columns are the snapshot selection's, and without the flag so are the static ones
    snap = select(torch, s, x0, ob, nbr)
    assert np.array_equal(got[:, ko:], snap[:, ko:])
    assert np.array_equal(select(torch, s, x0, ob, nbr, eps, False), snap)
    only = select(torch, s, x0, ob, nbr, eps, True, w, horizon, tables=1)
    assert np.array_equal(only[:, :ko], want) and (only[:, ko:] == -7).all()
    keys = sizes_oracle.clearance_keys(x0, ob, eps, s.params.Ts, N, w)
    if n_obs >= 63:
        assert (keys < 0).any() and (want != snap[:, :ko]).any()      # negative keys; the sizes matter in this world


@gpu
def test_clearance_selection_ties_nan_negative_levels_the_1000_m_rule_and_scenes():
    torch = _need_gpu()
    N, Ko = 10, 3
    s = solver(N, 2, Ko, 0)
    Ts = s.params.Ts
    x0 = np.array([[0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]])
    # rows 1 == 2: an exact tie (5 - 2), the lower index first; row 3 is the farthest centre but one and the second
    # smallest clearance (10 - 8); row 4 holds agent 0 inside its level set (1 - 2 < 0); row 5 has a NaN level and
    # row 6 a negative one: never selected, although their centres are the nearest
    ob = np.array([[9.0, 9.0], [3.0, 4.0], [3.0, 4.0], [10.0, 0.0], [1.0, 0.0], [0.5, 0.0], [0.2, 0.0]])
    eps = np.array([1.0, 4.0, 4.0, 64.0, 4.0, np.nan, -1.0])
    want = sizes_oracle.clearance_select(x0, ob, eps, Ko)
    assert want[0].tolist() == [4, 3, 1]
    assert sizes_oracle.clearance_keys(x0, ob, eps)[0, [1, 2, 3, 4]].tolist() == [3.0, 3.0, 2.0, -1.0]
    assert np.array_equal(select(torch, s, x0, ob, None, eps, True), want)
    s8 = solver(N, 2, 8, 0)                                  # fewer valid rows (5) than K_obs (7 after the clamp)
    want8 = sizes_oracle.clearance_select(x0, ob, eps, 8)
    assert want8[0].tolist() == [4, 3, 1, 2, 0, 0, 0]
    assert np.array_equal(select(torch, s8, x0, ob, None, eps, True), want8)
    # a NaN position; then nothing valid at all: every slot row 0
    obn = ob.copy()
    obn[4, 1] = np.nan
    wantn = sizes_oracle.clearance_select(x0, obn, eps, Ko)
    assert wantn[0].tolist() == [3, 1, 2]
    assert np.array_equal(select(torch, s, x0, obn, None, eps, True), wantn)
    nothing = np.full(7, np.nan)
    assert np.array_equal(select(torch, s, x0, ob, None, nothing, True), np.zeros((2, Ko), np.int32))
    # the 1000 m rule on the key: row 1's centre is 2000 m off and its level set 900 m; row 2's key is exactly 1000
    obf = np.array([[5.0, 0.0], [2000.0, 0.0], [0.0, 1500.0]])
    epsf = np.array([1.0, 1100.0 ** 2, 500.0 ** 2])
    wantf = sizes_oracle.clearance_select(x0[:1], obf, epsf, Ko)
    assert sizes_oracle.clearance_keys(x0[:1], obf, epsf)[0].tolist() == [4.0, 900.0, 1000.0]
    assert wantf[0].tolist() == [0, 1, 0]
    assert np.array_equal(select(torch, s, x0[:1], obf, None, epsf, True), wantf)
    # a row that comes close only later in the horizon, with horizon_selection
    vel = np.zeros((7, 2))
    obh = ob.copy()
    obh[0] = [64.0, 1.0]
    vel[0, 0] = -64.0 / (Ts * 8.0)                           # x = 0 at grid time Ts 8: distance 1, clearance 0
    wanth = sizes_oracle.clearance_select(x0, obh, eps, Ko, Ts, N, vel)
    assert wanth[0].tolist() == [4, 0, 3]
    assert np.array_equal(select(torch, s, x0, obh, None, eps, True, vel, True), wanth)
    # 3 scenes x 4 agents x 5 obstacles: global rows of the agent's scene, a shard inside a scene included
    S, sa, so = 3, 4, 5
    xs, nbs, obs_, vels = tmo.crossing_world(S * so, S * sa, 77)
    epss = np.random.default_rng(78).uniform(0.6, 3.6, S * so)
    epss[7] = np.nan                                          # a NaN level of scene 1
    obs_[10:15] += 5000.0                                     # scene 2 out of reach: its row 0 is global row 10
    u = srbnmpc.BatchSolver(srbnmpc.default_params(N, 2, K_obs=Ko, K_nbr=2), S * sa)
    try:
        u.set_scenes(sa, so)
        for w, hz in ((None, False), (vels, True)):
            wants = sizes_oracle.clearance_select(xs, obs_, epss, Ko, Ts, N, w, sa, so)
            assert (wants[2 * sa:] == 10).all() and not (wants[sa:2 * sa] == 7).any()
            assert ((wants[:sa] >= 0) & (wants[:sa] < so)).all() and ((wants[sa:2 * sa] >= so) & (wants[sa:2 * sa] < 2 * so)).all()
            gots = select(torch, u, xs, obs_, nbs, epss, True, w, hz)
            assert np.array_equal(gots[:, :Ko], wants)
            assert np.array_equal(gots[:, Ko:], select(torch, u, xs, obs_, nbs)[:, Ko:])
            part = select(torch, u, xs[2:7], obs_, nbs, epss, True, w, hz, agent_offset=2)
            assert np.array_equal(part, gots[2:7])
    finally:
        u.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_solve_with_the_clearance_selection_equals_the_oracle_handed_that_sel(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = sizes_oracle.reference(shape)
    b, eps = R["b"], np.array(R["eps"])
    s = solver(N, C, Ko, Kn)
    out = host_solve(s, b, obs_eps=eps, obs_clearance=True)
    assert np.array_equal(out["sel"], R["sel_c"])
    differ = int((out["sel"][:, :Ko] != R["r"]["sel"][:, :Ko]).any(1).sum())
    assert differ >= DIFFER_MIN[shape], differ
    assert_matches(N, C, out, R["rc"], f"{shape} clearance selection")
    d = device_solve(torch, s, b, obs_eps=eps, obs_clearance=True)
    for k in OUT_KEYS:
        assert np.array_equal(d[k], out[k]), k


# ---------------------------------------------------------------------------- 5. metrics
METRIC_KEYS = ("d_obs", "d_agent", "min_d_obs", "min_d_agent", "fail_cycle", "distance_to_fail")


def run_metrics(torch, s, states, ob, radius, agent_offset=0, n_agents=None, nbr=None):
    """srb_sim_metrics_sized_device (radius None: srb_sim_metrics_device) over the cycles states[c] [A][4], the
    neighbour table the states themselves (or nbr[c]); the host copies of the outputs after the last cycle."""
    A = states[0].shape[0] if n_agents is None else n_agents
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    m = dict(d_obs=torch.full((A,), 7.0, **f8), d_agent=torch.full((A,), 7.0, **f8), min_d_obs=torch.full((A,), 7.0, **f8),
             min_d_agent=torch.full((A,), 7.0, **f8), fail_cycle=torch.full((A,), 9, **i4),
             distance_to_fail=torch.full((A,), 7.0, **f8))
    t_ob = None if ob is None or ob.shape[0] == 0 else dev(torch, ob)
    t_r = None if radius is None else dev(torch, radius)
    P, I = srbnmpc._dptr, srbnmpc._iptr
    lib = srbnmpc.lib()
    for c, st in enumerate(states):
        t_st = dev(torch, st[agent_offset:agent_offset + A])
        full = st if nbr is None else nbr[c]
        t_nb = dev(torch, np.ascontiguousarray(full[:, [0, 2, 1, 3]]))
        sim = srbnmpc.Sim(state=P(t_st), obstacles=P(t_ob), nbr_state=P(t_nb), n_obs=0 if t_ob is None else ob.shape[0],
                          n_all=full.shape[0], agent_offset=agent_offset, d_obs=P(m["d_obs"]), d_agent=P(m["d_agent"]),
                          min_d_obs=P(m["min_d_obs"]), min_d_agent=P(m["min_d_agent"]), fail_cycle=I(m["fail_cycle"]),
                          distance_to_fail=P(m["distance_to_fail"]))
        if radius is None:
            srbnmpc._check(lib.srb_sim_metrics_device(s._h, A, ctypes.byref(sim), c, s._stream(None)))
        else:
            sz = srbnmpc.Sizes(None, P(t_r), 0)
            srbnmpc._check(lib.srb_sim_metrics_sized_device(s._h, A, ctypes.byref(sim), ctypes.byref(sz), c, s._stream(None)))
        torch.cuda.synchronize()
    return host(m)


def metric_world(n_obs, A, seed):
    """A agents over three cycles drifting through n_obs obstacles of radii U[0.1, 0.9] in a small arena, so that
    some cross a body and others never do."""
    g = np.random.default_rng(seed)
    side = 2.0 + np.sqrt(n_obs)
    ob = g.uniform(0, side, (n_obs, 2))
    rad = g.uniform(0.1, 0.9, n_obs)
    pos, v = g.uniform(0, side, (A, 2)), g.normal(0, 1.0, (A, 2))
    states = [np.ascontiguousarray(np.stack([pos[:, 0] + v[:, 0] * t, v[:, 0], pos[:, 1] + v[:, 1] * t, v[:, 1]], 1))
              for t in (0.0, 0.4, 0.8)]
    return states, ob, rad


@gpu
@pytest.mark.parametrize("n_obs", [1, 255, 256, 257])
def test_sized_metrics_equal_numpy_bitwise(n_obs):
    """Row counts around SIM_TILE = 256; 37 agents: three blocks of 16, the last one partly live."""
    torch = _need_gpu()
    s = solver(4, 4, 1, 0)
    A = 37
    states, ob, rad = metric_world(n_obs, A, 40 + n_obs)
    if n_obs > 1:
        ob[n_obs // 2, 0] = np.nan                           # a NaN row and a NaN radius never win
        rad[n_obs - 1] = np.nan
    m = sizes_oracle.Metrics(rad)
    for c, st in enumerate(states):
        m.update(c, st, ob, np.ascontiguousarray(st[:, [0, 2, 1, 3]]))
    got = run_metrics(torch, s, states, ob, rad)
    for k, v in m.as_dict().items():
        assert np.array_equal(got[k], v), k
    if n_obs >= 255:
        assert (got["fail_cycle"] >= 0).any() and (got["fail_cycle"] < 0).any() and (got["min_d_obs"] < 0).any()
    # the uniform 0.5 table: today's d_obs - 0.5 bit for bit, and today's fail_cycle
    half = np.full(n_obs, 0.5)
    plain, uni = run_metrics(torch, s, states, ob, None), run_metrics(torch, s, states, ob, half)
    assert np.array_equal(uni["d_obs"], plain["d_obs"] - 0.5) and np.array_equal(uni["min_d_obs"], plain["min_d_obs"] - 0.5)
    for k in ("fail_cycle", "distance_to_fail", "d_agent", "min_d_agent"):
        assert np.array_equal(uni[k], plain[k]), k
    # a shard of the team: rows 5 .. 25 of the neighbour table
    part = run_metrics(torch, s, states, ob, rad, agent_offset=5, n_agents=20)
    for k in METRIC_KEYS:
        assert np.array_equal(part[k], got[k][5:25]), k


@gpu
def test_sized_metrics_of_an_empty_table_and_of_scenes():
    torch = _need_gpu()
    s = solver(4, 4, 1, 0)
    states, ob, rad = metric_world(6, 5, 3)
    got = run_metrics(torch, s, states, None, rad)           # obs_radius beside n_obs = 0: +inf, nobody fails
    assert np.isinf(got["d_obs"]).all() and (got["d_obs"] > 0).all() and (got["fail_cycle"] == -1).all()
    allnan = run_metrics(torch, s, states, ob, np.full(6, np.nan))
    assert np.isinf(allnan["d_obs"]).all() and (allnan["fail_cycle"] == -1).all()
    # 3 scenes x 18 agents (two blocks a scene) x 7 obstacles against a per-scene numpy reference
    S, sa, so = 3, 18, 7
    states, ob, rad = metric_world(S * so, S * sa, 9)
    rad[8] = np.nan
    u = srbnmpc.BatchSolver(srbnmpc.default_params(4, 4, K_obs=1, K_nbr=0), S * sa)
    try:
        u.set_scenes(sa, so)
        got = run_metrics(torch, u, states, ob, rad)
        for g in range(S):
            m = sizes_oracle.Metrics(rad[g * so:(g + 1) * so])
            for c, st in enumerate(states):
                sg = st[g * sa:(g + 1) * sa]
                m.update(c, sg, ob[g * so:(g + 1) * so], np.ascontiguousarray(sg[:, [0, 2, 1, 3]]))
            for k, v in m.as_dict().items():
                assert np.array_equal(got[k][g * sa:(g + 1) * sa], v), (g, k)
        part = run_metrics(torch, u, states, ob, rad, agent_offset=11, n_agents=20)      # a shard across two scenes
        for k in METRIC_KEYS:
            assert np.array_equal(part[k], got[k][11:31]), k
    finally:
        u.close()


# ---------------------------------------------------------------------------- 6. rollout
_rolls = {}


def rollout(run, mode="run", moving=False, sizes="table", clear=False):
    """One of RUNS on the device with log_x, once per key: the host copies of results().  sizes: "table" the run's
    levels and radii, "uniform" eps_obs / 0.5 in every row, None no table."""
    key = (run, mode, moving, sizes, clear)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, C, Ko, Kn, T, seed = run
        state, goal, ob, w, eps, rad = sizes_oracle.world(run)
        if sizes == "uniform":
            eps, rad = np.full_like(eps, EPS_OBS), np.full_like(rad, 0.5)
        kw = {} if sizes is None else dict(obs_eps=dev(torch, eps), obs_radius=dev(torch, rad), obs_clearance=clear)
        if moving:
            kw.update(obs_vel=dev(torch, w), obs_horizon=clear)
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), log_x=True, obstacles=dev(torch, ob), **kw)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        _rolls[key] = host(r.results())
    return _rolls[key]


@gpu
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("run", RUNS)
def test_rollout_run_equals_steps_and_every_cycle_the_stand_alone_sized_solve(run, moving):
    torch = _need_gpu()
    A, N, C, Ko, Kn, T, seed = run
    a, b = rollout(run, "run", moving), rollout(run, "step", moving)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    state, goal, ob, vel, eps, rad = sizes_oracle.world(run)
    s = solver(N, C, Ko, Kn)
    p = s.params
    for c in range(T):
        obc = moving_oracle.advance_obstacles(p.Ts, ob, vel, c) if moving else ob
        bc, _ = sim_oracle.cycle_inputs(p, a["traj"][c], goal, obc, c)
        d = device_solve(torch, s, bc, obs_eps=eps, **(dict(obs_vel=vel) if moving else {}))
        assert np.array_equal(d["x"], a["x"][c]) and np.array_equal(d["status"], a["status"][c]), c
        assert np.array_equal(a["traj"][c + 1], sim_oracle.next_state(a["x"][c])), c


@gpu
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("run", RUNS)
def test_rollout_metrics_statuses_and_trajectories_against_the_sized_oracle(run, moving):
    """Cycle by cycle from the device's own trajectory, as the moving test does: the sized metrics bit for bit, the
    statuses equal and X, U, s of every cycle (so the next state) within 1e-4 of the sized oracle's closed-loop step."""
    _need_gpu()
    A, N, C, Ko, Kn, T, seed = run
    res = rollout(run, "run", moving)
    state, goal, ob, vel, eps, rad = sizes_oracle.world(run)
    p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    m = sizes_oracle.Metrics(rad, 0)
    worst = 0.0
    for c in range(T):
        obc = moving_oracle.advance_obstacles(p.Ts, ob, vel, c) if moving else ob
        bc, _ = sim_oracle.cycle_inputs(p, res["traj"][c], goal, obc, c)
        m.update(c, res["traj"][c], obc, bc["nbr_state"])
        o = sizes_oracle.solve(p, bc, eps, vel if moving else None)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        worst = max(worst, np.abs(xus(N, res["x"][c]) - xus(N, o["x"])).max())
        np.testing.assert_allclose(xus(N, res["x"][c]), xus(N, o["x"]), atol=tmo.NLP_TOL, rtol=0, err_msg=f"cycle {c}")
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), k
    print(f"run {run} moving={moving}: max |X,U,s - sized oracle| over {T} cycles = {worst:.3e}; min_d_obs smallest "
          f"{res['min_d_obs'].min():.4f} median {np.median(res['min_d_obs']):.4f}, "
          f"{int((res['fail_cycle'] >= 0).sum())} agents cross a body radius")


@gpu
@pytest.mark.parametrize("run", RUNS)
def test_a_uniform_table_rollout_equals_the_existing_rollout(run):
    for moving in (False, True):
        a, b = rollout(run, "run", moving, "uniform"), rollout(run, "run", moving, None)
        for k in b:
            if k in ("d_obs", "min_d_obs"):
                assert np.array_equal(a[k], b[k] - 0.5), (k, moving)
            else:
                assert np.array_equal(a[k], b[k]), (k, moving)
        # and the table matters: the sized world's trajectories are not the uniform world's
        assert not np.array_equal(rollout(run, "run", moving)["traj"], b["traj"])


@gpu
def test_rollout_with_the_clearance_selection():
    torch = _need_gpu()
    run = RUNS[0]
    A, N, C, Ko, Kn, T, seed = run
    state, goal, ob, vel, eps, rad = sizes_oracle.world(run)
    s = solver(N, C, Ko, Kn)
    for moving in (False, True):
        a, b = rollout(run, "run", moving, clear=True), rollout(run, "step", moving, clear=True)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, moving)
        w = vel if moving else None
        for c in (0, 1, T - 1):
            obc = moving_oracle.advance_obstacles(s.params.Ts, ob, vel, c) if moving else ob
            bc, _ = sim_oracle.cycle_inputs(s.params, a["traj"][c], goal, obc, c)
            kw = dict(obs_vel=vel, obs_horizon=True) if moving else {}
            d = device_solve(torch, s, bc, obs_eps=eps, obs_clearance=True, **kw)
            assert np.array_equal(d["x"], a["x"][c]), (c, moving)
            want = sizes_oracle.clearance_select(bc["x0"], obc, eps, Ko, s.params.Ts, N, w)
            assert np.array_equal(d["sel"][:, :Ko], want), (c, moving)


@gpu
@pytest.mark.parametrize("clear", [False, True])
def test_scene_batched_rollout_equals_the_per_team_rollouts(clear):
    """4 scenes x 4 agents, 5 obstacles each, 3 cycles, moving: one scene-batched run against four whole-team runs."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn, T, N, C = 4, 4, 5, 3, 3, 3, 10, 2
    b = workload.make_scenes(S, sa, N, C, seed=21, n_obs=so)
    vel = workload.obstacle_velocities(S * so, 21)
    eps, rad = workload.obstacle_sizes(S * so, 21)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), S * sa)
    u = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), S * sa)
    s.set_scenes(sa, so)
    f8 = torch.float64

    def roll(sol, rows, orows, mode="run"):
        r = srbnmpc.Rollout(sol, dev(torch, b["goal"][rows], f8), phase=dev(torch, b["phase"][rows], torch.int32),
                            obstacles=dev(torch, b["obstacles"][orows], f8), obs_vel=dev(torch, vel[orows], f8),
                            obs_horizon=clear, obs_eps=dev(torch, eps[orows], f8), obs_radius=dev(torch, rad[orows], f8),
                            obs_clearance=clear, log_x=True)
        r.reset(dev(torch, b["x0"][rows], f8))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = host(r.results())
        torch.cuda.synchronize()
        return res
    try:
        got = roll(s, slice(0, S * sa), slice(0, S * so))
        parts = [roll(u, slice(k * sa, (k + 1) * sa), slice(k * so, (k + 1) * so)) for k in range(S)]
        for k in got:
            if k == "cycles":
                continue
            axis = 1 if k in ("traj", "status", "iters", "x") else 0
            assert np.array_equal(got[k], np.concatenate([q[k] for q in parts], axis)), k
        stepped = roll(s, slice(0, S * sa), slice(0, S * so), "step")
        for k in got:
            assert np.array_equal(got[k], stepped[k]), k
    finally:
        s.close(); u.close()


@gpu
@pytest.mark.parametrize("clear", [False, True])
def test_four_shards_equal_the_full_batch(clear):
    """The stand-alone solve in four agent_offset shards, and four Rollout shards of run 0 stepping in lockstep (the
    all-gather stood in for by torch.cat) against the full team: metrics, logs and trajectories."""
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = sizes_oracle.reference(SHAPE_C2)
    b, eps = R["b"], np.array(R["eps"])
    s = solver(N, C, Ko, Kn)
    full = host_solve(s, b, obs_eps=eps, obs_clearance=clear)
    for r in range(4):
        lo, hi = sdist.shard_range(A, 4, r)
        part = s.solve(b["x0"][lo:hi], b["ref"][lo:hi], b["foot"][lo:hi], b["obstacles"], b["nbr_state"],
                       agent_offset=lo, obs_eps=eps, obs_clearance=clear)
        dpart = device_solve(torch, s, b, agent_offset=lo, rows=slice(lo, hi), obs_eps=eps, obs_clearance=clear)
        for k in OUT_KEYS:
            assert np.array_equal(part[k], full[k][lo:hi]), (k, r)
            assert np.array_equal(dpart[k], full[k][lo:hi]), ("device", k, r)
    run = RUNS[0]
    A, N, C, Ko, Kn, T, seed = run
    want = rollout(run, "run", True, clear=clear)
    state, goal, ob, vel, eps, rad = sizes_oracle.world(run)
    sh = []
    for r in range(4):
        lo, hi = sdist.shard_range(A, 4, r)
        u = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), hi - lo)
        q = srbnmpc.Rollout(u, dev(torch, goal[lo:hi]), log_x=True, obstacles=dev(torch, ob), obs_vel=dev(torch, vel),
                            obs_horizon=clear, obs_eps=dev(torch, eps), obs_radius=dev(torch, rad), obs_clearance=clear,
                            agent_offset=lo, n_all=A)
        q.reset(dev(torch, state[lo:hi]))
        sh.append(q)
    try:
        cycles = 3
        for _ in range(cycles):
            for q in sh:
                q.advance()
            table = torch.cat([q.last_state for q in sh]).contiguous()
            for q in sh:
                q.step(exchange=lambda local, table=table: table)
        got = [host(q.results()) for q in sh]
        for k in ("traj", "status", "iters", "x"):
            assert np.array_equal(np.concatenate([g[k] for g in got], 1), want[k][:cycles + 1 if k == "traj" else cycles]), k
        # the metrics after three cycles: the sized numpy metrics over the full team's trajectory
        m = sizes_oracle.Metrics(rad, 0)
        for c in range(cycles):
            st = want["traj"][c]
            m.update(c, st, moving_oracle.advance_obstacles(sh[0].solver.params.Ts, ob, vel, c),
                     np.ascontiguousarray(st[:, [0, 2, 1, 3]]))
        for k, v in m.as_dict().items():
            assert np.array_equal(np.concatenate([g[k] for g in got]), v), k
    finally:
        for q in sh:
            q.solver.close()


# ---------------------------------------------------------------------------- 7. refusals
@gpu
def test_refusals_by_name_with_a_live_context_and_nothing_is_launched():
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = sizes_oracle.reference(SHAPE_C2)
    b, eps = R["b"], np.array(R["eps"])
    s = solver(N, C, Ko, Kn)
    good = host_solve(s, b, obs_eps=eps)
    lib = srbnmpc.lib()
    keep, cases = _refusal_cases()
    for entry, sz, word in cases:
        assert _call_refused(lib, s._h, entry, sz) == -1, (entry, word)
        assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())
    # through the Python layer, with real device buffers: the outputs stay untouched
    t = {k: dev(torch, b[k]) for k in ("x0", "ref", "obstacles", "nbr_state")}
    t["foot"] = dev(torch, np.asarray(b["foot"]).reshape(A, -1))
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o = dict(x=torch.full((A, s.params.nv), 7.0, **f8), obj=torch.zeros(A, **f8), status=torch.full((A, 2), 9, **i4),
             iters=torch.zeros(A, 2, **i4))
    de = dev(torch, eps)
    sel = torch.full((A, Ko + Kn), -7, **i4)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs obs_eps") as e:
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_clearance=True)
    assert "srbnmpc error -1:" in str(e.value)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs obs_eps"):
        host_solve(s, b, obs_clearance=True)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs obs_eps"):
        s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, obs_clearance=True)
    with pytest.raises(RuntimeError, match="horizon_selection = 1 needs obs_vel"):
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_eps=de, obs_horizon=True)
    with pytest.raises(RuntimeError, match="obstacles_version"):                    # srb_moving's refusal stands
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_eps=de,
                       obs_vel=dev(torch, np.zeros_like(b["obstacles"])), obstacles_version=3)
    torch.cuda.synchronize()
    assert (o["x"] == 7.0).all() and (o["status"] == 9).all() and (sel == -7).all()
    for name, kw in (("obs_eps", dict(obs_eps=de[:-1])), ("obs_eps", dict(obs_eps=de.float())), ("obs_eps", dict(obs_eps=de.cpu()))):
        with pytest.raises(ValueError, match=name):
            s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, **kw)
    with pytest.raises(ValueError, match="obs_eps"):
        host_solve(s, b, obs_eps=eps.astype(np.float32))
    with pytest.raises(ValueError, match="QP-only"):
        host_solve(s, b, obs_eps=eps, qp_only=True)
    goal = dev(torch, np.zeros((A, 2)))
    with pytest.raises(ValueError, match="obs_clearance needs obs_eps"):
        srbnmpc.Rollout(s, goal, obstacles=t["obstacles"], obs_clearance=True)
    with pytest.raises(ValueError, match="obs_radius needs obstacles"):
        srbnmpc.Rollout(s, goal, obs_radius=de)
    with pytest.raises(ValueError, match="obs_radius"):
        srbnmpc.Rollout(s, goal, obstacles=t["obstacles"], obs_radius=de[:-1])
    with pytest.raises(ValueError, match="obs_eps"):
        srbnmpc.Rollout(s, goal, obstacles=t["obstacles"], obs_eps=de.cpu())
    assert (o["x"] == 7.0).all() and (o["status"] == 9).all()
    # obs_eps goes together with a versioned table: the grid of centres is built once and the bits are the same
    o2 = dict(x=torch.zeros(A, s.params.nv, **f8), obj=torch.zeros(A, **f8), status=torch.zeros(A, 2, **i4),
              iters=torch.zeros(A, 2, **i4), sel=torch.full((A, Ko + Kn), -7, **i4))
    s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o2, obs_eps=de, obstacles_version=5)
    torch.cuda.synchronize()
    assert np.array_equal(o2["x"].cpu().numpy(), good["x"]) and np.array_equal(o2["sel"].cpu().numpy(), good["sel"])
    again = host_solve(s, b, obs_eps=eps)                                    # the context survives
    for k in OUT_KEYS:
        assert np.array_equal(again[k], good[k]), k
