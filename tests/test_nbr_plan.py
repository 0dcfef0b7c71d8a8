"""Neighbour plans for the inter-agent CBF rows: srb_batch.nbr_plan / plan (ABI 6), the horizon-aware
neighbour selection (SRB_OPT_PLAN_SELECTION) and the outer-iteration driver solve_coupled_device.

Tolerances are those of tests/test_gpu_parity.py: statuses exact; X, U, s within NLP_TOL = 1e-4 (the full x
too when C = 2); obj at rtol 1e-7 / atol 1e-6; iteration counts equal for at least 85 % of the agents and
never off by more than 2.  The reference is tests/plan_oracle.py: the oracle's own chain per agent, with the
neighbour columns of its obstacle rows taken from the plan table.  The shapes (plan_oracle.SHAPES) are the
smallest that reach every code path: the generic instance, the compiled configs[2] instance, the N = 20
instance with folded obstacle rows and its separate polish kernel, and C = 4.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

import oracle
import plan_oracle
import srbnmpc
from srbnmpc import dist as sdist

NLP_TOL = 1e-4
SHAPES = plan_oracle.SHAPES
SHAPE_C2 = SHAPES[1]                      # (10, 2, 3 + 8, 64 agents): the compiled configs[2] instance

gpu = pytest.mark.gpu


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def moved(shape):
    """Agents whose X, U differ by more than 1e-3 between the plan oracle and the constant-velocity oracle."""
    R = plan_oracle.reference(shape)
    N = shape[0]
    return (np.abs(R["r1"]["x"][:, :6 * N] - R["r0"]["x"][:, :6 * N]).max(1) > 1e-3).sum()


# ============================================================================================ CPU
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_helper_equals_oracle_batch_with_constant_velocity_table(shape):
    """plan_oracle.solve with table = pos + vel * Ts (k + 1) is oracle.solve_batch, bit for bit."""
    R = plan_oracle.reference(shape)
    r = plan_oracle.solve(R["p"], R["b"], plan_oracle.cv_table(R["p"], R["b"]["nbr_state"]))
    for k in ("x_qp", "x", "status", "iters"):
        assert np.array_equal(r[k], R["r0"][k]), k
    np.testing.assert_allclose(r["obj"], R["r0"]["obj"], rtol=1e-12)
    # and the helper's selection is the oracle's
    assert r["sel"].shape == (shape[4], shape[2] + shape[3])


def test_abi_version_6_everywhere():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert srbnmpc.lib().srb_abi_version() == 6 and srbnmpc.ABI_VERSION == 6
    assert "#define SRB_OPT_PLAN_SELECTION %d\n" % srbnmpc.OPTIONS["plan_selection"] in hdr
    assert srbnmpc.OPTIONS["plan_selection"] == 14


def test_batch_layout_matches_the_header(tmp_path):
    """sizeof(srb_batch) and the offsets of the two new members, from the system C compiler, against the
    ctypes mirror."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(srb_batch), offsetof(srb_batch, nbr_plan), '
                   'offsetof(srb_batch, plan), offsetof(srb_batch, obstacles_version)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    B = srbnmpc.Batch
    assert got == [ctypes.sizeof(B), B.nbr_plan.offset, B.plan.offset, B.obstacles_version.offset]
    assert B._fields_[-2][0] == "nbr_plan" and B._fields_[-1][0] == "plan"        # appended after obstacles_version
    assert srbnmpc.Batch().struct_size == ctypes.sizeof(B)


def test_shift_plans():
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(3)
    t = torch.randn(7, 6, 2, dtype=torch.float64, generator=g)
    s0 = sdist.shift_plans(t, 0)
    assert torch.equal(s0, t) and s0.data_ptr() != t.data_ptr()
    # a straight line with coordinates representable in binary: exact for every shift, past the horizon too
    n, N = 5, 6
    p0 = torch.tensor([[1.0, -2.0], [0.5, 0.25], [-3.0, 8.0], [0.0, 0.0], [16.0, -0.125]], dtype=torch.float64)
    v = torch.tensor([[0.25, 0.5], [-1.0, 2.0], [0.0, 0.125], [3.0, -0.75], [-0.5, -0.5]], dtype=torch.float64)
    k = torch.arange(1, N + 1, dtype=torch.float64).view(1, N, 1)
    line = p0[:, None, :] + v[:, None, :] * k
    for g_ in (1, 2, 5, 6, 9):
        assert torch.equal(sdist.shift_plans(line, g_), p0[:, None, :] + v[:, None, :] * (k + g_)), g_
    # a curved plan: the kept grids are copies, the tail continues the last finite difference
    s2 = sdist.shift_plans(t, 2)
    assert torch.equal(s2[:, :4], t[:, 2:])
    d = t[:, 5] - t[:, 4]
    assert torch.equal(s2[:, 4], t[:, 5] + 1.0 * d) and torch.equal(s2[:, 5], t[:, 5] + 2.0 * d)


def test_python_layer_validates_plan_arrays_before_the_library():
    """Shape / dtype / contiguity of nbr_plan and plan are checked the way out['sel'] is."""
    with pytest.raises(ValueError, match="nbr_plan"):
        srbnmpc._check_plan_array(np.zeros((4, 10, 2), np.float32), (4, 10, 2), "nbr_plan", np.float64)
    with pytest.raises(ValueError, match="plan"):
        srbnmpc._check_plan_array(np.zeros((4, 10, 3)), (4, 10, 2), "plan", np.float64)
    with pytest.raises(ValueError, match="plan"):
        srbnmpc._check_plan_array(np.zeros((4, 10, 4))[:, :, ::2], (4, 10, 2), "plan", np.float64)
    srbnmpc._check_plan_array(np.zeros((4, 10, 2)), (4, 10, 2), "plan", np.float64)


# ============================================================================================ GPU
def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_solvers = {}


def solver(N, C, Ko, Kn, use_nlp=1, max_agents=512):
    key = (N, C, Ko, Kn, use_nlp, max_agents)
    if key not in _solvers:
        _solvers[key] = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), max_agents)
    return _solvers[key]


def host_solve(s, b, **kw):
    return s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], **kw)


def assert_matches(N, C, out, r, what):
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


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_plans_against_the_oracle(shape):
    """solve(nbr_plan = the oracle's round-0 plans) == the plan oracle; the table matters (the answer moves
    by more than 1e-3 on several agents), so a solve that ignored it would fail."""
    _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = plan_oracle.reference(shape)
    assert moved(shape) >= (4 if shape == SHAPE_C2 else 1), moved(shape)
    s = solver(N, C, Ko, Kn)
    out = host_solve(s, R["b"], nbr_plan=R["table"])
    assert_matches(N, C, out, R["r1"], f"{shape}")
    assert np.array_equal(out["sel"], R["r1"]["sel"])
    assert np.array_equal(out["plan"], plan_oracle.plans_of(R["p"], out["x"]))


@gpu
@pytest.mark.parametrize("variant", ["waves1", "waves2", "waves4", "polish_kernel"])
def test_plans_against_the_oracle_every_wave_count_and_the_polish_kernel(variant):
    _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        if variant == "polish_kernel":
            s.set_option("polish_fused", 0)
        else:
            s.set_waves(int(variant[-1]))
        out = host_solve(s, R["b"], nbr_plan=R["table"])
        if variant == "polish_kernel":
            assert s.get_option("last_polish") == 1.0
        else:
            assert s.waves() == int(variant[-1])
        assert_matches(N, C, out, R["r1"], variant)
        assert np.array_equal(out["plan"], plan_oracle.plans_of(R["p"], out["x"]))
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_velocity_table_equals_the_plain_solve(shape):
    """A numpy constant-velocity table gives the statuses of the plain solve and x within NLP_TOL of it (the
    table's p + v t is rounded once where the kernel may fuse the multiply-add: round-off only is expected)."""
    _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = plan_oracle.reference(shape)
    s = solver(N, C, Ko, Kn)
    plain = host_solve(s, R["b"])
    out = host_solve(s, R["b"], nbr_plan=plan_oracle.cv_table(R["p"], R["b"]["nbr_state"]))
    print(f"{shape}: max |x(cv table) - x(plain)| = {np.abs(out['x'] - plain['x']).max():.3e}")
    assert np.array_equal(out["status"], plain["status"])
    np.testing.assert_allclose(out["x"], plain["x"], atol=NLP_TOL, rtol=0)


def _device_batch(torch, b):
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device="cuda") for k in ("x0", "ref", "foot", "obstacles", "nbr_state")}
    t["foot"] = t["foot"].reshape(t["x0"].shape[0], -1).contiguous()
    return t


def _device_out(torch, A, p, with_plan=True):
    o = dict(x_qp=torch.zeros(A, p.nv, dtype=torch.float64, device="cuda"),
             x=torch.zeros(A, p.nv, dtype=torch.float64, device="cuda"),
             obj=torch.zeros(A, dtype=torch.float64, device="cuda"),
             status=torch.zeros(A, 2, dtype=torch.int32, device="cuda"),
             iters=torch.zeros(A, 2, dtype=torch.int32, device="cuda"))
    if with_plan:
        o["plan"] = torch.full((A, p.N, 2), float("nan"), dtype=torch.float64, device="cuda")
    return o


def _device_solve(torch, s, t, o, **kw):
    s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
@pytest.mark.parametrize("fused", [1, 0])
def test_plan_output_is_the_gather_of_x(shape, fused):
    """plan == (x[4k], x[4k + 2]) of the returned x, bitwise: host and device paths, the fused polish and the
    polish kernel (which rewrites x after the solve kernel wrote it), with and without a table."""
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = shape
    R = plan_oracle.reference(shape)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        s.set_option("polish_fused", fused)
        for table in (None, R["table"]):
            out = host_solve(s, R["b"], nbr_plan=table)
            if not fused:
                assert s.get_option("last_polish") == 1.0
            assert np.array_equal(out["plan"], plan_oracle.plans_of(R["p"], out["x"]))
            t = _device_batch(torch, R["b"])
            o = _device_out(torch, A, s.params)
            dev = _device_solve(torch, s, t, o, nbr_plan=None if table is None else torch.as_tensor(np.array(table), device="cuda"))
            assert np.array_equal(dev["plan"], plan_oracle.plans_of(R["p"], dev["x"]))
            assert np.array_equal(dev["x"], out["x"]) and np.array_equal(dev["plan"], out["plan"])
    finally:
        s.close()


@gpu
def test_plan_output_of_the_qp_only_solve():
    """srb_solve_qp writes plan from the QP x and ignores nbr_plan."""
    _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    s = solver(N, C, Ko, Kn)
    a = host_solve(s, R["b"], qp_only=True)
    b = host_solve(s, R["b"], qp_only=True, nbr_plan=R["table"])
    assert np.array_equal(a["plan"], plan_oracle.plans_of(R["p"], a["x"]))
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["plan"], b["plan"])
    assert np.abs(a["plan"]).max() > 0.0


@gpu
@pytest.mark.parametrize("shards", [2, 8])
def test_shards_with_the_full_table_equal_the_full_batch(shards):
    _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    b = R["b"]
    s = solver(N, C, Ko, Kn)
    full = host_solve(s, b, nbr_plan=R["table"])
    for r in range(shards):
        lo, hi = sdist.shard_range(A, shards, r)
        part = s.solve(b["x0"][lo:hi], b["ref"][lo:hi], b["foot"][lo:hi], b["obstacles"], b["nbr_state"],
                       agent_offset=lo, nbr_plan=R["table"])
        for k in ("x_qp", "x", "obj", "status", "iters", "sel", "plan"):
            assert np.array_equal(part[k], full[k][lo:hi]), (k, r)


# ---------------------------------------------------------------------------- horizon-aware selection
def crossing_tables(n_all, N, seed, Ts=0.043):
    """Synthetic crossing plans: random starts in an arena that grows with the swarm, fast velocities and a
    curvature term, so agents that are distant now pass close later.  Returns x0 [n,4], nbr_state [n,4],
    plan [n,N,2] (row k at time Ts (k + 1))."""
    rng = np.random.default_rng(seed)
    side = 2.0 * np.sqrt(n_all)
    pos = rng.uniform(0, side, (n_all, 2))
    vel = rng.normal(0, 12.0, (n_all, 2))
    acc = rng.normal(0, 40.0, (n_all, 2))
    t = Ts * np.arange(1, N + 1)
    plan = pos[:, None] + vel[:, None] * t[None, :, None] + 0.5 * acc[:, None] * (t * t)[None, :, None]
    nbr = np.concatenate([pos, vel], 1)
    x0 = np.stack([pos[:, 0], vel[:, 0], pos[:, 1], vel[:, 1]], 1)
    return np.ascontiguousarray(x0), np.ascontiguousarray(nbr), np.ascontiguousarray(plan)


def brute_force(x0, nbr, plan, Kn, lo=0, hi=None, horizon=True):
    """The selection as the header defines it: key d_i = sqrt(min_k (dx_k^2 + dy_k^2)) over the snapshot pair
    (k = 0) and the N plan pairs, a stable sort on (d, index), row g excluded, NaN rows never selected, -1
    where fewer than Kn rows remain.  horizon=False: the snapshot key alone (the existing selection)."""
    n_all = nbr.shape[0]
    hi = x0.shape[0] + lo if hi is None else hi
    out = np.full((hi - lo, Kn), -1, np.int32)
    for a in range(hi - lo):
        g = lo + a
        dx, dy = x0[a, 0] - nbr[:, 0], x0[a, 2] - nbr[:, 1]
        d2 = dx * dx + dy * dy
        if horizon:
            ex, ey = plan[g, :, 0][None] - plan[:, :, 0], plan[g, :, 1][None] - plan[:, :, 1]
            d2 = np.min(np.concatenate([d2[:, None], ex * ex + ey * ey], 1), 1)      # NaN propagates
        d = np.sqrt(d2)
        idx = np.array([i for i in np.lexsort((np.arange(n_all), d)) if i != g and not np.isnan(d[i])], np.int32)
        out[a, :min(Kn, idx.size)] = idx[:Kn]
    return out


def _select(torch, s, x0, ob, nbr, plan, tables=3, plan_selection=1, lo=0, sel=None):
    Ko, Kn = s.n_selected(ob.shape[0], nbr.shape[0])
    if sel is None:
        sel = torch.full((x0.shape[0], Ko + Kn), -7, dtype=torch.int32, device="cuda")
    s.set_option("plan_selection", plan_selection)
    try:
        s.select_device(torch.as_tensor(x0, device="cuda"), torch.as_tensor(ob, device="cuda"),
                        torch.as_tensor(nbr, device="cuda"), sel, tables=tables, agent_offset=lo,
                        nbr_plan=None if plan is None else torch.as_tensor(plan, device="cuda"))
        torch.cuda.synchronize()
    finally:
        s.set_option("plan_selection", 0)
    return sel


@gpu
@pytest.mark.parametrize("n_all", [5, 64, 300])
@pytest.mark.parametrize("Kn", [2, 8, 16])
def test_horizon_aware_selection_against_brute_force(n_all, Kn):
    """n_all = 5 with K_nbr 8 or 16 is the n_all - 1 < K_nbr case: the C ABI clamps the neighbour columns to
    the n_all - 1 rows that exist (as for the snapshot selection), so every other agent is selected, in key
    order; the -1 fill itself is reached through rows that cannot be selected (the NaN test below)."""
    torch = _need_gpu()
    N, Ko = 10, 3
    x0, nbr, plan = crossing_tables(n_all, N, seed=100 + n_all)
    ob = np.random.default_rng(1).uniform(0, 10, (7, 2))
    s = solver(N, 2, Ko, Kn)
    kn = min(Kn, n_all - 1)
    ref = brute_force(x0, nbr, plan, kn)
    snap = brute_force(x0, nbr, plan, kn, horizon=False)
    got = _select(torch, s, x0, ob, nbr, plan).cpu().numpy()
    assert got.shape == (n_all, Ko + kn)
    assert np.array_equal(got[:, Ko:], ref), np.where((got[:, Ko:] != ref).any(1))[0]
    # the static columns are the existing kernel's, and the snapshot selection is untouched by the option
    old = _select(torch, s, x0, ob, nbr, None, plan_selection=0).cpu().numpy()
    st = _select(torch, s, x0, ob, nbr, None, tables=1, plan_selection=0).cpu().numpy()
    assert np.array_equal(got[:, :Ko], st[:, :Ko]) and np.array_equal(old[:, :Ko], st[:, :Ko])
    assert np.array_equal(old[:, Ko:], snap)
    # split selection around a collective: tables = 1, then tables = 2 into the same tensor == one pass
    sel = _select(torch, s, x0, ob, nbr, plan, tables=1)
    assert (sel[:, Ko:] == -7).all()
    sel = _select(torch, s, x0, ob, nbr, plan, tables=2, sel=sel).cpu().numpy()
    assert np.array_equal(sel, got)
    if n_all == 64:
        differ = sum(set(ref[a]) != set(snap[a]) for a in range(n_all))
        assert differ >= n_all // 4, differ
    # a shard of the swarm: agent_offset
    if n_all == 300:
        lo, hi = 137, 201
        part = _select(torch, s, x0[lo:hi], ob, nbr, plan, lo=lo).cpu().numpy()
        assert np.array_equal(part, got[lo:hi])


@gpu
def test_horizon_aware_selection_ties_nan_rows_and_the_solve():
    torch = _need_gpu()
    N, Ko, Kn = 10, 3, 2
    s = solver(N, 2, Ko, Kn)
    ob = np.array([[50.0, 50.0], [60.0, 50.0], [70.0, 50.0]])
    # exactly representable coordinates.  Agent 0 rests at the origin; rows 1 and 2 rest at distance 5 on
    # opposite sides (an exact tie: the lower index wins); row 3 starts far away and passes at distance 1 at
    # grid 4; row 4 is nearest now (distance 4) and leaves.
    n_all = 6
    plan = np.zeros((n_all, N, 2))
    nbr = np.zeros((n_all, 4))
    nbr[1, :2] = (3.0, 4.0); nbr[2, :2] = (-3.0, -4.0); nbr[3, :2] = (64.0, 1.0); nbr[4, :2] = (0.0, 4.0)
    nbr[5, :2] = (100.0, 100.0)
    plan[:] = nbr[:, None, :2]
    plan[3, :, 0] = 64.0 - 16.0 * np.arange(1, N + 1)          # x = 0 at grid 4 (k = 3): distance 1
    plan[4, :, 1] = 4.0 + 8.0 * np.arange(1, N + 1)
    x0 = np.stack([nbr[:, 0], 0 * nbr[:, 0], nbr[:, 1], 0 * nbr[:, 0]], 1)
    ref = brute_force(x0, nbr, plan, Kn)
    assert ref[0].tolist() == [3, 4]                            # closest approach 1, then the snapshot's 4
    got = _select(torch, s, x0, ob, nbr, plan).cpu().numpy()
    assert np.array_equal(got[:, Ko:], ref)
    # the tie alone: rows 3 and 4 out of reach
    far = plan.copy(); far[3] += 1000.0; far[4] += 1000.0
    nbr2 = nbr.copy(); nbr2[3, :2] += 1000.0; nbr2[4, :2] += 1000.0
    x02 = np.stack([nbr2[:, 0], 0 * nbr2[:, 0], nbr2[:, 1], 0 * nbr2[:, 0]], 1)
    ref2 = brute_force(x02, nbr2, far, Kn)
    assert ref2[0].tolist() == [1, 2]
    got2 = _select(torch, s, x02, ob, nbr2, far).cpu().numpy()
    assert np.array_equal(got2[:, Ko:], ref2)
    # rows with a NaN anywhere in their plan or snapshot are never selected: fewer than Kn rows remain -> -1
    x0n, nbrn, plann = crossing_tables(4, N, seed=9)
    plann[1, 7, 1] = np.nan
    nbrn[2, 0] = np.nan
    refn = brute_force(x0n, nbrn, plann, Kn)
    assert refn[0].tolist() == [3, -1] and refn[3].tolist() == [0, -1]
    gotn = _select(torch, s, x0n, ob, nbrn, plann).cpu().numpy()
    assert np.array_equal(gotn[:, Ko:], refn)
    # the solve runs the same selection (SRB_OPT_PLAN_SELECTION = 1, SRB_OPT_SELECTION = 1)
    N2, C2, Ko2, Kn2, A2, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    b = R["b"]
    s2 = solver(N2, C2, Ko2, Kn2)
    table = np.ascontiguousarray(R["table"])
    want = brute_force(b["x0"], b["nbr_state"], table, Kn2)
    s2.set_option("plan_selection", 1)
    try:
        out = host_solve(s2, b, nbr_plan=table)
    finally:
        s2.set_option("plan_selection", 0)
    assert np.array_equal(out["sel"][:, Ko2:], want)
    assert np.array_equal(out["sel"][:, :Ko2], R["r1"]["sel"][:, :Ko2])
    r = plan_oracle.solve(R["p"], b, table, sel=out["sel"])
    assert_matches(N2, C2, out, r, "plan selection + plans")


# ---------------------------------------------------------------------------- the driver
@gpu
def test_coupled_driver_equals_manual_rounds():
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    s = solver(N, C, Ko, Kn)
    t = _device_batch(torch, R["b"])
    # three manual rounds with explicit tables
    rounds = []
    table = None
    for r in range(3):
        o = _device_out(torch, A, s.params)
        rounds.append(_device_solve(torch, s, t, o, nbr_plan=table))
        table = o["plan"]
    # round 0 is the plain solve, round 1 the solve against round 0's plans: the oracle's first Jacobi step
    assert_matches(N, C, rounds[1], plan_oracle.solve(R["p"], R["b"], rounds[0]["plan"]), "round 1")
    o = _device_out(torch, A, s.params)
    change = s.solve_coupled_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, outer=3)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert np.array_equal(v.cpu().numpy(), rounds[2][k]), k
    want = [np.abs(rounds[r]["plan"] - rounds[r - 1]["plan"]).max() for r in (1, 2)]
    assert change.shape == (2,) and change.is_cuda and change.cpu().tolist() == want
    assert want[0] > 1e-3                                      # the iteration moves the plans at all
    # outer = 1 is solve_device
    o1 = _device_out(torch, A, s.params)
    c1 = s.solve_coupled_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o1, outer=1)
    torch.cuda.synchronize()
    assert c1.numel() == 0
    for k, v in o1.items():
        assert np.array_equal(v.cpu().numpy(), rounds[0][k]), k
    # outer = 2 with a table for round 0
    o2 = _device_out(torch, A, s.params)
    s.solve_coupled_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o2, outer=2,
                           nbr_plan=torch.as_tensor(rounds[0]["plan"], device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(o2["x"].cpu().numpy(), rounds[2]["x"])


@gpu
def test_coupled_driver_through_a_one_rank_rccl_exchange():
    """The driver with exchange = PlanExchange on a one-rank RCCL group (force_collective), in a child process
    (the group must not outlive the test): the same results as without the exchange."""
    _need_gpu()
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    code = f"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'srb-cbf-nmpc_amd')!r}]
import srbnmpc
from srbnmpc import dist as sd, workload
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="{port}")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
N, C, Ko, Kn, A, seed = {SHAPE_C2!r}
b = workload.make_batch(A, N, C, seed=seed)
s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
t = {{k: torch.as_tensor(np.ascontiguousarray(b[k]), device="cuda") for k in ("x0", "ref", "foot", "obstacles", "nbr_state")}}
t["foot"] = t["foot"].reshape(A, -1).contiguous()
def outs():
    return dict(x_qp=torch.zeros(A, s.params.nv, dtype=torch.float64, device="cuda"),
                x=torch.zeros(A, s.params.nv, dtype=torch.float64, device="cuda"),
                obj=torch.zeros(A, dtype=torch.float64, device="cuda"),
                status=torch.zeros(A, 2, dtype=torch.int32, device="cuda"),
                iters=torch.zeros(A, 2, dtype=torch.int32, device="cuda"),
                plan=torch.zeros(A, N, 2, dtype=torch.float64, device="cuda"))
o0, o1 = outs(), outs()
c0 = s.solve_coupled_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o0, outer=3)
ex = sd.PlanExchange(A, 1, 0, torch.device("cuda", 0), N, force_collective=True)
c1 = s.solve_coupled_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o1, outer=3, exchange=ex)
torch.cuda.synchronize()
assert ex.sets[0].flat and ex.turn == 0
for k in o0:
    assert torch.equal(o0[k], o1[k]), k
assert torch.equal(c0, c1) and float(c0[0]) > 1e-3
dist.destroy_process_group()
print("coupled rccl ok")
"""
    r = subprocess.run([sys.executable, "-c", code], timeout=150, capture_output=True, text=True)
    assert r.returncode == 0 and "coupled rccl ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------- refusals
@gpu
def test_argument_errors_are_refused_by_name_and_the_context_survives():
    torch = _need_gpu()
    N, C, Ko, Kn, A, _ = SHAPE_C2
    R = plan_oracle.reference(SHAPE_C2)
    b = R["b"]
    s = solver(N, C, Ko, Kn)
    table = np.array(R["table"])
    good = host_solve(s, b, nbr_plan=table)

    def refused(msg, fn):
        with pytest.raises(RuntimeError, match=msg) as e:
            fn()
        assert "srbnmpc error -1:" in str(e.value)              # SRB_ERR_ARG
        again = host_solve(s, b, nbr_plan=table)                # a following valid solve succeeds
        assert np.array_equal(again["x"], good["x"]) and np.array_equal(again["status"], good["status"])

    # nbr_plan without nbr_state (host and device paths)
    refused("nbr_plan needs nbr_state",
            lambda: s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], None, nbr_plan=table))
    t = _device_batch(torch, b)
    o = _device_out(torch, A, s.params)
    dt = torch.as_tensor(table, device="cuda")
    refused("nbr_plan needs nbr_state",
            lambda: s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], None, o, nbr_plan=dt))
    # agent_offset + n_agents > n_all with a plan table
    refused("agent_offset",
            lambda: s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, nbr_plan=dt,
                                   agent_offset=1))
    # plan overlapping the table: the table itself, and a window that shares its last rows
    refused("plan overlaps the nbr_plan table",
            lambda: s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, nbr_plan=dt, plan=dt))
    big = torch.zeros(2 * A - 1, N, 2, dtype=torch.float64, device="cuda")
    refused("plan overlaps the nbr_plan table",
            lambda: s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o,
                                   nbr_plan=big[:A], plan=big[A - 1:]))
    refused("plan overlaps the nbr_plan table",
            lambda: s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nbr_plan=table, plan=table))
    # adjacent, not overlapping: accepted
    big2 = torch.zeros(2 * A, N, 2, dtype=torch.float64, device="cuda")
    big2[:A] = dt
    s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o, nbr_plan=big2[:A], plan=big2[A:])
    torch.cuda.synchronize()
    assert np.array_equal(o["x"].cpu().numpy(), good["x"])
    # horizon-aware selection without a table: the solve and the selection alone
    s.set_option("plan_selection", 1)
    try:
        refused_sel = "SRB_OPT_PLAN_SELECTION = 1 needs nbr_plan"
        with pytest.raises(RuntimeError, match=refused_sel):
            host_solve(s, b)
        with pytest.raises(RuntimeError, match=refused_sel):
            s.solve_device(t["x0"], t["ref"], t["foot"], t["obstacles"], t["nbr_state"], o)
        sel = torch.zeros(A, Ko + Kn, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match=refused_sel):
            s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, tables=2)
        s.select_device(t["x0"], t["obstacles"], t["nbr_state"], sel, tables=1)      # needs no table
        with pytest.raises(RuntimeError, match="SRB_OPT_PLAN_SELECTION: 0"):
            s.set_option("plan_selection", 2)
    finally:
        s.set_option("plan_selection", 0)
    again = host_solve(s, b, nbr_plan=table)
    assert np.array_equal(again["x"], good["x"])
