"""Moving obstacles: srb_moving (obs_vel, horizon_selection) through the selection, the solve and the rollout.

The reference is tests/moving_oracle.py: the oracle's own chain per agent with the static columns of its obstacle
rows moved at the table's velocities, and numpy restatements of the horizon-aware obstacle selection and of the
obstacle advance.  Tolerances are the project's (tests/test_gpu_parity.py, test_nbr_plan.assert_matches): statuses
equal; X, U, s within 1e-4 (the full x too at C = 2); obj at rtol 1e-7 / atol 1e-6; iterations equal on at least
85 % of the agents and never off by more than 2.  Selections, the advance, "off is off", run == steps, shards and
scenes are compared bit for bit.  The shapes are plan_oracle.SHAPES: the generic instance, the compiled configs[2]
instance, the N = 20 folded instance with its separate polish kernel, and C = 4.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import moving_oracle
import plan_oracle
import sim_oracle
import srbnmpc
from srbnmpc import dist as sdist
from srbnmpc import workload

NLP_TOL = 1e-4
SHAPES = plan_oracle.SHAPES
SHAPE_C2 = SHAPES[1]
MOVED_MIN = dict(zip(SHAPES, (4, 16, 4, 4)))          # agents the table must move by > 1e-3 (measured 8 / 39 / 10 / 11)
DIFFER_MIN = dict(zip(SHAPES, (1, 8, 4, 1)))          # agents whose horizon selection must differ (measured 1 / 32 / 12 / 3)
OUT_KEYS = ("x", "x_qp", "obj", "status", "iters", "sel")
gpu = pytest.mark.gpu
_dp = ctypes.POINTER(ctypes.c_double)


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def assert_matches(N, C, out, r, what):
    """The project's solve tolerances (tests/test_nbr_plan.py assert_matches, tests/test_gpu_parity.py)."""
    bad = np.where((out["status"] != r["status"]).any(1))[0]
    assert bad.size == 0, (what, [(int(a), out["status"][a].tolist(), r["status"][a].tolist()) for a in bad])
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max()
    print(f"{what}: max |X,U,s - oracle| = {e:.3e}, iterations equal on "
          f"{np.mean(np.all(out['iters'] == r['iters'], 1)):.3f}")
    assert np.mean(np.all(out["iters"] == r["iters"], 1)) >= 0.85, what
    assert np.abs(out["iters"] - r["iters"]).max() <= 2, what
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0, err_msg=what)
    if C == 2:
        np.testing.assert_allclose(out["x"], r["x"], atol=NLP_TOL, rtol=0, err_msg=what)
    np.testing.assert_allclose(out["obj"], r["obj"], rtol=1e-7, atol=1e-6, err_msg=what)


# ============================================================================================ CPU
@pytest.mark.parametrize("shape", SHAPES)
def test_helper_with_a_zero_table_equals_oracle_batch(shape):
    R = plan_oracle.reference(shape)
    r = moving_oracle.solve(R["p"], R["b"], np.zeros_like(R["b"]["obstacles"]))
    for k in ("x_qp", "x", "status", "iters"):
        assert np.array_equal(r[k], R["r0"][k]), k


def test_moving_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(srb_moving), offsetof(srb_moving, struct_size), '
                   'offsetof(srb_moving, obs_vel), offsetof(srb_moving, horizon_selection), offsetof(srb_moving, obstacles));'
                   ' return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = srbnmpc.Moving
    assert got == [ctypes.sizeof(M), M.struct_size.offset, M.obs_vel.offset, M.horizon_selection.offset, M.obstacles.offset]
    assert srbnmpc.Moving().struct_size == ctypes.sizeof(M)


def test_abi_version_is_still_6_and_the_old_layouts_stand():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert srbnmpc.lib().srb_abi_version() == 6 and srbnmpc.ABI_VERSION == 6
    assert srbnmpc.Batch._fields_[-1][0] == "plan" and srbnmpc.Sim._fields_[-1][0] == "distance_to_fail"


def test_obstacle_velocities_are_deterministic_and_bounded():
    for n, seed, vmax in ((20, 5, 1.0), (320, 12, 0.5), (1, 0, 2.0)):
        v = workload.obstacle_velocities(n, seed, vmax)
        assert v.shape == (n, 2) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"]
        assert np.array_equal(v, workload.obstacle_velocities(n, seed, vmax))
        sp = np.sqrt((v * v).sum(1))
        assert (sp >= 0.25 * vmax * (1 - 1e-12)).all() and (sp <= vmax * (1 + 1e-12)).all()
        g = np.random.default_rng(100 + seed)
        s0 = g.uniform(0.25 * vmax, vmax, n)
        th = g.uniform(0, 2 * np.pi, n)
        assert np.array_equal(v, np.stack([s0 * np.cos(th), s0 * np.sin(th)], 1))
    assert not np.array_equal(workload.obstacle_velocities(20, 5), workload.obstacle_velocities(20, 6))
    assert np.array_equal(workload.obstacle_velocities(20, 5), workload.obstacle_velocities(20, 5, vmax=1.0))


def test_python_layer_validates_obs_vel_by_name():
    chk = srbnmpc._check_vel_array
    with pytest.raises(ValueError, match="obs_vel"):
        chk(np.zeros((4, 2), np.float32), 4, np.float64)
    with pytest.raises(ValueError, match="obs_vel"):
        chk(np.zeros((5, 2)), 4, np.float64)
    with pytest.raises(ValueError, match="obs_vel"):
        chk(np.zeros((4, 4))[:, ::2], 4, np.float64)
    with pytest.raises(ValueError, match="obs_vel"):
        chk([[0.0, 0.0]] * 4, 4, np.float64)
    chk(np.zeros((4, 2)), 4, np.float64)


def _refusal_cases():
    """(entry, word) of every refusal of srb_moving that needs no context: the checks run before the context is
    looked at, so a null context reaches them (with a live context nothing is launched either: the GPU test)."""
    vel = np.zeros((3, 2))
    ob = np.zeros((3, 2))
    other = np.zeros((3, 2))
    pv, po, px = (a.ctypes.data_as(_dp) for a in (vel, ob, other))
    keep = (vel, ob, other)
    B, M, S = srbnmpc.Batch, srbnmpc.Moving, srbnmpc.Sim

    def batch(version=0):
        b = B()
        b.obstacles, b.n_obs, b.obstacles_version = po, 3, version
        return b
    bad_size = M(pv, 0, None)
    bad_size.struct_size += 8
    return keep, [
        ("solve", batch(), bad_size, "srb_moving.struct_size"),
        ("solve", batch(7), M(pv, 0, None), "obstacles_version"),
        ("solve", batch(), M(None, 1, None), "horizon_selection = 1 needs obs_vel"),
        ("rollout", batch(), M(pv, 0, None), "srb_moving.obstacles missing"),
        ("rollout", batch(), M(pv, 0, px), "is not srb_batch.obstacles"),
        ("rollout", batch(7), M(pv, 0, po), "obstacles_version"),
        ("rollout", batch(), bad_size, "srb_moving.struct_size"),
    ]


def _call_refused(lib, h, entry, b, mv, n_agents=1):
    sim = srbnmpc.Sim()
    if entry == "rollout":
        return lib.srb_rollout_moving_device(h, n_agents, ctypes.byref(b), ctypes.byref(sim), ctypes.byref(mv), 1, None)
    rcs = {lib.srb_solve_batch_moving(h, n_agents, ctypes.byref(b), ctypes.byref(mv)),
           lib.srb_solve_batch_moving_device(h, n_agents, ctypes.byref(b), ctypes.byref(mv), None),
           lib.srb_select_moving_device(h, n_agents, ctypes.byref(b), ctypes.byref(mv), 1, None)}
    assert len(rcs) == 1, rcs
    return rcs.pop()


def test_refusals_by_name_without_a_context():
    lib = srbnmpc.lib()
    keep, cases = _refusal_cases()
    for entry, b, mv, word in cases:
        assert _call_refused(lib, None, entry, b, mv) == -1, (entry, word)
        assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())


def test_oracle_closed_loop_in_the_moving_world():
    """The smallest of the issue's runs, oracle only: every agent-cycle OPTIMAL, aware and unaware; the smallest
    and median min_d_obs the issue records for it (0.183 / 0.710 aware, 0.150 / 0.677 unaware)."""
    run = moving_oracle.RUNS[2]
    for aware, lo, med in ((True, 0.183, 0.710), (False, 0.150, 0.677)):
        L = moving_oracle.closed_loop(run, aware)
        assert (L["status"][..., 1] == 0).all() and np.isin(L["status"][..., 0], (0, 4)).all()
        d = L["metrics"]["min_d_obs"]
        print(f"aware={aware}: min_d_obs smallest {d.min():.4f} median {np.median(d):.4f}")
        assert abs(d.min() - lo) < 6e-4 and abs(np.median(d) - med) < 6e-4


# ============================================================================================ GPU
def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, C, Ko, Kn, max_agents=64):
    key = (N, C, Ko, Kn, max_agents)
    if key not in _solvers:
        _solvers[key] = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), max_agents)
    return _solvers[key]


def dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def host_solve(s, b, **kw):
    return s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], **kw)


def device_solve(torch, s, b, agent_offset=0, rows=slice(None), **kw):
    """solve_device on the host batch b (rows: the agents of a shard); every keyword that is an array goes to the
    device.  Returns the host copies of the outputs, sel included."""
    x0 = np.asarray(b["x0"]).reshape(-1, 4)[rows]
    A = x0.shape[0]
    t = dict(x0=dev(torch, x0), ref=dev(torch, np.asarray(b["ref"]).reshape(-1, 4 * s.params.N)[rows]),
             foot=dev(torch, np.asarray(b["foot"]).reshape(len(b["x0"]), -1)[rows]),
             obstacles=dev(torch, b["obstacles"]), nbr_state=None if b.get("nbr_state") is None else dev(torch, b["nbr_state"]))
    p = s.params
    Ko, Kn = s.n_selected(t["obstacles"].shape[0], 0 if t["nbr_state"] is None else t["nbr_state"].shape[0])
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o = dict(x_qp=torch.zeros(A, p.nv, **f8), x=torch.zeros(A, p.nv, **f8), obj=torch.zeros(A, **f8),
             status=torch.zeros(A, 2, **i4), iters=torch.zeros(A, 2, **i4), sel=torch.full((A, Ko + Kn), -7, **i4))
    kw = {k: (dev(torch, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, agent_offset=agent_offset, **kw)
    torch.cuda.synchronize()
    return host(o)


def moved_agents(shape):
    R = moving_oracle.reference(shape)
    N = shape[0]
    return int((np.abs(R["r"]["x"][:, :6 * N] - R["r0"]["x"][:, :6 * N]).max(1) > 1e-3).sum())


# ---------------------------------------------------------------------------- 1. off is off
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_a_zero_table_gives_the_bits_of_the_call_without_one(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    b = plan_oracle.reference(shape)["b"]
    s = solver(N, C, Ko, Kn)
    zero = np.zeros_like(b["obstacles"])
    plain, off = host_solve(s, b), host_solve(s, b, obs_vel=zero)
    for k in OUT_KEYS:
        assert np.array_equal(plain[k], off[k]), ("host", k)
    dplain, doff = device_solve(torch, s, b), device_solve(torch, s, b, obs_vel=zero)
    for k in OUT_KEYS:
        assert np.array_equal(dplain[k], doff[k]), ("device", k)
        assert np.array_equal(dplain[k], plain[k]), ("host / device", k)


# ---------------------------------------------------------------------------- 2. against the oracle
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_moving_table_against_the_oracle(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = moving_oracle.reference(shape)
    assert moved_agents(shape) >= MOVED_MIN[shape], moved_agents(shape)          # the table matters
    s = solver(N, C, Ko, Kn)
    out = host_solve(s, R["b"], obs_vel=np.array(R["vel"]))
    assert_matches(N, C, out, R["r"], f"{shape} host")
    assert np.array_equal(out["sel"], R["r"]["sel"])
    d = device_solve(torch, s, R["b"], obs_vel=np.array(R["vel"]))
    for k in OUT_KEYS:
        assert np.array_equal(d[k], out[k]), k


@gpu
def test_moving_table_with_neighbour_plans_against_the_oracle():
    _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = moving_oracle.reference(SHAPE_C2)
    table = np.array(plan_oracle.reference(SHAPE_C2)["table"])
    r = moving_oracle.solve(R["p"], R["b"], R["vel"], table=table)
    s = solver(N, C, Ko, Kn)
    out = host_solve(s, R["b"], obs_vel=np.array(R["vel"]), nbr_plan=table)
    assert_matches(N, C, out, r, "moving table + plans")
    # both tables matter: neither the plan-only nor the velocity-only answer
    for other in (plan_oracle.reference(SHAPE_C2)["r1"], R["r"]):
        assert (np.abs(xus(N, out["x"]) - xus(N, other["x"])).max(1) > 1e-3).sum() >= 4


# ---------------------------------------------------------------------------- 3. read only through sel
@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_the_velocity_table_is_read_only_through_sel(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = moving_oracle.reference(shape)
    s = solver(N, C, Ko, Kn)
    vel = np.array(R["vel"])
    good = host_solve(s, R["b"], obs_vel=vel)
    used = np.unique(good["sel"][:, :min(Ko, vel.shape[0])])
    assert used.size < vel.shape[0]
    holes = vel.copy()
    holes[np.setdiff1d(np.arange(vel.shape[0]), used)] = np.nan
    for out in (host_solve(s, R["b"], obs_vel=holes), device_solve(torch, s, R["b"], obs_vel=holes)):
        for k in OUT_KEYS:
            assert np.array_equal(out[k], good[k]), k


# ---------------------------------------------------------------------------- 4. horizon-aware selection
def _obs_waves():
    """SRB_KNN_OBS_WAVES of csrc/srb_kernel_params.h: one pass of the kernel's scan covers 64 x this many rows."""
    import re
    hdr = open(os.path.join(ROOT, "srb-cbf-nmpc_amd", "csrc", "srb_kernel_params.h")).read()
    return int(re.search(r"#define SRB_KNN_OBS_WAVES (\d+)", hdr).group(1))


WAVES = _obs_waves()


def crossing_world(n_obs, A, seed, N=10):
    """Agents and obstacles whose order of approach changes over the horizon: fast, in a small arena."""
    g = np.random.default_rng(seed)
    side = 1.0 + np.sqrt(n_obs)
    ob = g.uniform(0, side, (n_obs, 2))
    vel = g.normal(0, 6.0, (n_obs, 2))
    pos = g.uniform(0, side, (A, 2))
    v = g.normal(0, 3.0, (A, 2))
    x0 = np.stack([pos[:, 0], v[:, 0], pos[:, 1], v[:, 1]], 1)
    nbr = np.stack([pos[:, 0], pos[:, 1], v[:, 0], v[:, 1]], 1)
    return np.ascontiguousarray(x0), np.ascontiguousarray(nbr), ob, vel


def select(torch, s, x0, ob, nbr, vel=None, horizon=False, tables=3, agent_offset=0):
    Ko, Kn = s.n_selected(ob.shape[0], 0 if nbr is None else nbr.shape[0])
    sel = torch.full((x0.shape[0], Ko + Kn), -7, dtype=torch.int32, device="cuda")
    s.select_device(dev(torch, x0), dev(torch, ob), None if nbr is None else dev(torch, nbr), sel, tables=tables,
                    agent_offset=agent_offset, obs_vel=None if vel is None else dev(torch, vel), obs_horizon=horizon)
    torch.cuda.synchronize()
    return sel.cpu().numpy()


@gpu
@pytest.mark.parametrize("n_obs", [1, 3, 63, 64, 65, 64 * WAVES - 1, 64 * WAVES, 64 * WAVES + 1])
@pytest.mark.parametrize("Ko", [1, 3, 8])
def test_horizon_selection_index_for_index(n_obs, Ko):
    """Every row count either side of a lane, a wave and a scan pass (64 x the kernel's wave count); K_obs 1, 3, 8,
    and K_obs > n_obs (n_obs 1 and 3), which clamps to the rows that exist."""
    torch = _need_gpu()
    N, A, Kn = 10, 9, 2
    s = solver(N, 2, Ko, Kn)
    x0, nbr, ob, vel = crossing_world(n_obs, A, 1000 * Ko + n_obs)
    want = moving_oracle.horizon_select(s.params.Ts, N, x0, ob, vel, Ko)
    got = select(torch, s, x0, ob, nbr, vel, True)
    ko = min(Ko, n_obs)
    assert got.shape == (A, ko + Kn) and want.shape == (A, ko)
    assert np.array_equal(got[:, :ko], want), np.where((got[:, :ko] != want).any(1))[0]
    # the neighbour columns are the snapshot selection's, and without the flag so are the static ones
    snap = select(torch, s, x0, ob, nbr)
    assert np.array_equal(got[:, ko:], snap[:, ko:])
    assert np.array_equal(select(torch, s, x0, ob, nbr, vel, False), snap)
    assert np.array_equal(snap[:, :ko], moving_oracle.select_by_key(moving_oracle.snapshot_keys(x0, ob), Ko))
    # tables = 1 writes the static columns alone
    only = select(torch, s, x0, ob, nbr, vel, True, tables=1)
    assert np.array_equal(only[:, :ko], want) and (only[:, ko:] == -7).all()
    if n_obs >= 63:
        assert (want != snap[:, :ko]).any()                  # the horizon matters in this world


@gpu
def test_horizon_selection_ties_nan_rows_the_1000_m_rule_and_scenes():
    torch = _need_gpu()
    N, Ko = 10, 3
    s = solver(N, 2, Ko, 0)
    Ts = s.params.Ts
    x0 = np.array([[0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]])
    # duplicate rows (1 == 2, 4 == 5): the lower index first; row 3 is far now and passes close later
    ob = np.array([[9.0, 9.0], [3.0, 4.0], [3.0, 4.0], [64.0, 1.0], [-3.0, -4.0], [-3.0, -4.0]])
    vel = np.zeros((6, 2))
    vel[3, 0] = -64.0 / (Ts * 8.0)                           # x = 0 at grid time Ts 8: distance 1
    want = moving_oracle.horizon_select(Ts, N, x0, ob, vel, Ko)
    assert want[0].tolist() == [3, 1, 2]
    assert np.array_equal(select(torch, s, x0, ob, None, vel, True), want)
    vel0 = np.zeros((6, 2))
    want0 = moving_oracle.horizon_select(Ts, N, x0, ob, vel0, Ko)
    assert want0[0].tolist() == [1, 2, 4]
    assert np.array_equal(select(torch, s, x0, ob, None, vel0, True), want0)
    # NaN in a position and in a velocity: never selected; with fewer valid rows than K_obs the rest is row 0
    obn, veln = ob.copy(), vel.copy()
    obn[1, 1] = np.nan
    veln[3, 0] = np.nan
    wantn = moving_oracle.horizon_select(Ts, N, x0, obn, veln, Ko)
    assert wantn[0].tolist() == [2, 4, 5]
    assert np.array_equal(select(torch, s, x0, obn, None, veln, True), wantn)
    obn[[2, 4, 5], 0] = np.nan
    wantn = moving_oracle.horizon_select(Ts, N, x0, obn, veln, Ko)
    assert wantn[0].tolist()[1:] == [0, 0] and wantn[0, 0] == 0
    assert np.array_equal(select(torch, s, x0, obn, None, veln, True), wantn)
    # an obstacle at >= 1000 m for its whole horizon gets row 0; one that comes within 1000 m is selected
    obf = np.array([[5.0, 0.0], [2000.0, 0.0], [0.0, 1500.0], [1001.0, 0.0]])
    velf = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, -1.0], [-10.0, 0.0]])
    wantf = moving_oracle.horizon_select(Ts, N, x0, obf, velf, Ko)
    assert wantf[0].tolist() == [0, 3, 0]
    assert np.array_equal(select(torch, s, x0, obf, None, velf, True), wantf)
    # 3 scenes x 4 agents x 5 obstacles: global rows of the agent's scene, a shard inside a scene included
    S, sa, so = 3, 4, 5
    xs, nbs, obs_, vels = crossing_world(S * so, S * sa, 77)
    vels[7] = np.nan                                          # a NaN row of scene 1
    obs_[10:15] += 5000.0                                     # scene 2 out of reach: its row 0 is global row 10
    u = srbnmpc.BatchSolver(srbnmpc.default_params(N, 2, K_obs=Ko, K_nbr=2), S * sa)
    try:
        u.set_scenes(sa, so)
        wants = moving_oracle.horizon_select(Ts, N, xs, obs_, vels, Ko, sa, so)
        assert (wants[2 * sa:] == 10).all() and not (wants[sa:2 * sa] == 7).any()
        gots = select(torch, u, xs, obs_, nbs, vels, True)
        assert np.array_equal(gots[:, :Ko], wants)
        assert np.array_equal(gots[:, Ko:], select(torch, u, xs, obs_, nbs)[:, Ko:])
        part = select(torch, u, xs[2:7], obs_, nbs, vels, True, agent_offset=2)
        assert np.array_equal(part, gots[2:7])
    finally:
        u.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_solve_with_the_horizon_selection_equals_the_oracle_handed_that_sel(shape):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = moving_oracle.reference(shape)
    b, p, vel = R["b"], R["p"], np.array(R["vel"])
    s = solver(N, C, Ko, Kn)
    want = moving_oracle.horizon_select(p.Ts, N, b["x0"], b["obstacles"], vel, Ko)
    out = host_solve(s, b, obs_vel=vel, obs_horizon=True)
    snap = host_solve(s, b, obs_vel=vel)
    assert np.array_equal(out["sel"][:, :Ko], want)
    assert np.array_equal(out["sel"][:, Ko:], snap["sel"][:, Ko:])
    differ = int((out["sel"][:, :Ko] != snap["sel"][:, :Ko]).any(1).sum())
    assert differ >= DIFFER_MIN[shape], differ
    r = moving_oracle.solve(p, b, vel, sel=out["sel"])
    assert_matches(N, C, out, r, f"{shape} horizon selection")
    d = device_solve(torch, s, b, obs_vel=vel, obs_horizon=True)
    for k in OUT_KEYS:
        assert np.array_equal(d[k], out[k]), k


# ---------------------------------------------------------------------------- 5. obstacle advance
@gpu
@pytest.mark.parametrize("n_obs", [1, 255, 256, 257])
def test_obstacle_advance_equals_numpy_bitwise(n_obs):
    torch = _need_gpu()
    s = solver(4, 4, 1, 0)
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


# ---------------------------------------------------------------------------- 6. rollout
_rolls = {}


def rollout(run, mode="run", plans=False, vel="table"):
    """One of moving_oracle.RUNS on the device with log_x, once per key: the host copies of results().  vel:
    "table" the run's velocities, "zero" a zero table, None no table."""
    key = (run, mode, plans, vel)
    if key not in _rolls:
        torch = _need_gpu()
        A, N, C, Ko, Kn, T, seed = run
        state, goal, ob, w = moving_oracle.world(run)
        v = None if vel is None else dev(torch, w if vel == "table" else np.zeros_like(w))
        table = dev(torch, ob)
        r = srbnmpc.Rollout(solver(N, C, Ko, Kn), dev(torch, goal), plans=plans, log_x=True, obstacles=table, obs_vel=v)
        r.reset(dev(torch, state))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = host(r.results())
        if vel is not None:
            assert np.array_equal(table.cpu().numpy(), ob)                 # the caller's table stays
            r.reset(dev(torch, state))
            assert np.array_equal(r.obstacles.cpu().numpy(), ob)           # reset() restores the start table
        _rolls[key] = res
    return _rolls[key]


@gpu
@pytest.mark.parametrize("run", moving_oracle.RUNS)
def test_rollout_run_equals_steps_and_every_cycle_the_stand_alone_solve(run):
    torch = _need_gpu()
    A, N, C, Ko, Kn, T, seed = run
    a, b = rollout(run, "run"), rollout(run, "step")
    assert sorted(a) == sorted(b) and "obstacles" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    state, goal, ob, vel = moving_oracle.world(run)
    s = solver(N, C, Ko, Kn)
    p = s.params
    assert np.array_equal(a["obstacles"], moving_oracle.advance_obstacles(p.Ts, ob, vel, T - 1))
    assert not np.array_equal(a["obstacles"], ob)
    for c in range(T):
        bc, _ = sim_oracle.cycle_inputs(p, a["traj"][c], goal, moving_oracle.advance_obstacles(p.Ts, ob, vel, c), c)
        d = device_solve(torch, s, bc, obs_vel=vel)
        assert np.array_equal(d["x"], a["x"][c]) and np.array_equal(d["status"], a["status"][c]), c
        assert np.array_equal(a["traj"][c + 1], sim_oracle.next_state(a["x"][c])), c


@gpu
@pytest.mark.parametrize("run", moving_oracle.RUNS)
def test_rollout_metrics_and_every_cycle_against_the_moving_oracle(run):
    _need_gpu()
    A, N, C, Ko, Kn, T, seed = run
    res = rollout(run)
    state, goal, ob, vel = moving_oracle.world(run)
    import oracle
    p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    m = sim_oracle.Metrics(0)
    worst = 0.0
    for c in range(T):
        obc = moving_oracle.advance_obstacles(p.Ts, ob, vel, c)
        bc, _ = sim_oracle.cycle_inputs(p, res["traj"][c], goal, obc, c)
        m.update(c, res["traj"][c], obc, bc["nbr_state"])
        o = moving_oracle.solve(p, bc, vel)
        assert np.array_equal(res["status"][c], o["status"]), (c, res["status"][c].tolist(), o["status"].tolist())
        worst = max(worst, np.abs(xus(N, res["x"][c]) - xus(N, o["x"])).max())
        np.testing.assert_allclose(xus(N, res["x"][c]), xus(N, o["x"]), atol=NLP_TOL, rtol=0, err_msg=f"cycle {c}")
    for k, v in m.as_dict().items():
        assert np.array_equal(res[k], v), k
    print(f"run {run}: max |X,U,s - moving oracle| over {T} cycles = {worst:.3e}; min_d_obs smallest "
          f"{res['min_d_obs'].min():.4f} median {np.median(res['min_d_obs']):.4f}")


@gpu
@pytest.mark.parametrize("run", moving_oracle.RUNS)
def test_a_zero_table_rollout_equals_the_existing_rollout(run):
    a, b = rollout(run, "run", vel="zero"), rollout(run, "run", vel=None)
    assert "obstacles" not in b
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    # and the table matters: the moving world's trajectories are not the static world's
    assert not np.array_equal(rollout(run)["traj"], b["traj"])


@gpu
def test_rollout_with_plans_in_the_moving_world():
    torch = _need_gpu()
    run = moving_oracle.RUNS[0]
    A, N, C, Ko, Kn, T, seed = run
    a, b = rollout(run, "run", plans=True), rollout(run, "step", plans=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["x"], rollout(run)["x"])                   # the plans are in use
    state, goal, ob, vel = moving_oracle.world(run)
    import oracle
    p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    for c in (0, 1, T - 1):
        obc = moving_oracle.advance_obstacles(p.Ts, ob, vel, c)
        bc, table = sim_oracle.cycle_inputs(p, a["traj"][c], goal, obc, c, a["x"][c - 1] if c else None, True)
        o = moving_oracle.solve(p, bc, vel, table=table)
        assert np.array_equal(a["status"][c], o["status"]), c
        np.testing.assert_allclose(xus(N, a["x"][c]), xus(N, o["x"]), atol=NLP_TOL, rtol=0, err_msg=f"cycle {c}")


@gpu
@pytest.mark.parametrize("horizon", [False, True])
def test_scene_batched_rollout_equals_the_per_team_rollouts(horizon):
    """4 scenes x 4 agents, 5 obstacles each, 3 cycles: one scene-batched run against four whole-team runs."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn, T, N, C = 4, 4, 5, 3, 3, 3, 10, 2
    b = workload.make_scenes(S, sa, N, C, seed=21, n_obs=so)
    vel = workload.obstacle_velocities(S * so, 21)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), S * sa)
    u = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), S * sa)
    s.set_scenes(sa, so)
    f8 = torch.float64

    def roll(sol, rows, orows, mode="run"):
        r = srbnmpc.Rollout(sol, dev(torch, b["goal"][rows], f8), phase=dev(torch, b["phase"][rows], torch.int32),
                            obstacles=dev(torch, b["obstacles"][orows], f8), obs_vel=dev(torch, vel[orows], f8),
                            obs_horizon=horizon, log_x=True)
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
        assert np.array_equal(got["obstacles"], moving_oracle.advance_obstacles(s.params.Ts, b["obstacles"], vel, T - 1))
    finally:
        s.close(); u.close()


# ---------------------------------------------------------------------------- 7. shards
@gpu
@pytest.mark.parametrize("horizon", [False, True])
def test_four_shards_equal_the_full_batch(horizon):
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = moving_oracle.reference(SHAPE_C2)
    b, vel = R["b"], np.array(R["vel"])
    s = solver(N, C, Ko, Kn)
    full = host_solve(s, b, obs_vel=vel, obs_horizon=horizon)
    for r in range(4):
        lo, hi = sdist.shard_range(A, 4, r)
        part = s.solve(b["x0"][lo:hi], b["ref"][lo:hi], b["foot"][lo:hi], b["obstacles"], b["nbr_state"],
                       agent_offset=lo, obs_vel=vel, obs_horizon=horizon)
        dpart = device_solve(torch, s, b, agent_offset=lo, rows=slice(lo, hi), obs_vel=vel, obs_horizon=horizon)
        for k in OUT_KEYS:
            assert np.array_equal(part[k], full[k][lo:hi]), (k, r)
            assert np.array_equal(dpart[k], full[k][lo:hi]), ("device", k, r)


@gpu
def test_rollout_shards_move_their_own_copy_of_the_table():
    """Two shards of run 0 stepping in lockstep (the all-gather stood in for by torch.cat) against the full team."""
    torch = _need_gpu()
    run = moving_oracle.RUNS[0]
    A, N, C, Ko, Kn, T, seed = run
    want = rollout(run, "run")
    state, goal, ob, vel = moving_oracle.world(run)
    cut, sh = 7, []
    for lo, hi in ((0, cut), (cut, A)):
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), hi - lo)
        r = srbnmpc.Rollout(s, dev(torch, goal[lo:hi]), log_x=True, obstacles=dev(torch, ob), obs_vel=dev(torch, vel),
                            agent_offset=lo, n_all=A)
        r.reset(dev(torch, state[lo:hi]))
        sh.append(r)
    try:
        for _ in range(3):
            for r in sh:
                r.advance()
            table = torch.cat([r.last_state for r in sh]).contiguous()
            for r in sh:
                r.step(exchange=lambda local, table=table: table)
        got = [host(r.results()) for r in sh]
        for k in ("traj", "status", "iters", "x"):
            assert np.array_equal(np.concatenate([g[k] for g in got], 1), want[k][:4 if k == "traj" else 3]), k
        for g in got:
            assert np.array_equal(g["obstacles"], moving_oracle.advance_obstacles(sh[0].solver.params.Ts, ob, vel, 2))
    finally:
        for r in sh:
            r.solver.close()


# ---------------------------------------------------------------------------- 8. refusals
@gpu
def test_refusals_by_name_with_a_live_context_and_nothing_is_launched():
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = moving_oracle.reference(SHAPE_C2)
    b, vel = R["b"], np.array(R["vel"])
    s = solver(N, C, Ko, Kn)
    good = host_solve(s, b, obs_vel=vel)
    lib = srbnmpc.lib()
    keep, cases = _refusal_cases()
    for entry, bt, mv, word in cases:
        assert _call_refused(lib, s._h, entry, bt, mv) == -1, (entry, word)
        assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())
    # through the Python layer, with real device buffers: the outputs stay untouched
    t = {k: dev(torch, b[k]) for k in ("x0", "ref", "obstacles", "nbr_state")}
    t["foot"] = dev(torch, np.asarray(b["foot"]).reshape(A, -1))
    f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o = dict(x=torch.full((A, s.params.nv), 7.0, **f8), obj=torch.zeros(A, **f8), status=torch.full((A, 2), 9, **i4),
             iters=torch.zeros(A, 2, **i4))
    dv = dev(torch, vel)
    with pytest.raises(RuntimeError, match="obstacles_version") as e:
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_vel=dv, obstacles_version=3)
    assert "srbnmpc error -1:" in str(e.value)
    with pytest.raises(RuntimeError, match="horizon_selection = 1 needs obs_vel"):
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_horizon=True)
    with pytest.raises(RuntimeError, match="horizon_selection = 1 needs obs_vel"):
        host_solve(s, b, obs_horizon=True)
    sel = torch.full((A, Ko + Kn), -7, **i4)
    with pytest.raises(RuntimeError, match="horizon_selection = 1 needs obs_vel"):
        s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, obs_horizon=True)
    with pytest.raises(RuntimeError, match="obstacles_version"):
        s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, obs_vel=dv, obs_horizon=True, obstacles_version=3)
    torch.cuda.synchronize()
    assert (o["x"] == 7.0).all() and (o["status"] == 9).all() and (sel == -7).all()
    with pytest.raises(ValueError, match="obs_vel"):
        s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, obs_vel=dv[:-1])
    with pytest.raises(ValueError, match="obs_vel"):
        host_solve(s, b, obs_vel=vel.astype(np.float32))
    with pytest.raises(ValueError, match="obs_horizon needs obs_vel"):
        srbnmpc.Rollout(s, dev(torch, np.zeros((A, 2))), obstacles=t["obstacles"], obs_horizon=True)
    with pytest.raises(ValueError, match="obs_vel needs obstacles"):
        srbnmpc.Rollout(s, dev(torch, np.zeros((A, 2))), obs_vel=dv)
    again = host_solve(s, b, obs_vel=vel)                                   # the context survives
    for k in OUT_KEYS:
        assert np.array_equal(again[k], good[k]), k
