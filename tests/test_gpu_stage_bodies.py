"""GPU tests of the solve kernel's stage bodies (csrc/srb_kernels.hip nmpc_agent, csrc/srb_stage_body.h): the compiled
one-column-block instances 12_4_1_10_2_11 and 12_1_4_10_2_3 (and their mv / f32 forms) carry one copy of the stage body
for the QP stage and one for the NLP stage, each with `nl` a constant; every other instance keeps the one loop over
the two stages.  What can go wrong is what the two copies no longer share: the QP copy alone, the hand-off between
the copies (the QP point, the slots' state, the LDS buffers), the polish that follows the NLP copy, state that
survives from one solve or one stage into the next -- and the run-time instances, which an earlier form of the split
broke (N = 11 on 12_4_1_0_0_0, N = 12 on 24_5_1_0_0_0) and which are machine-code identical to their one-loop form now.

Comparison rule, as tests/test_gpu_factor_chain.py: statuses equal, iteration counts equal, X, U, s within 1e-4,
within 1e-6 where both sides end NLP OPTIMAL (at least one agent must).

All batches are workload.make_batch.  Oracle facts the cases rest on (asserted below, on the oracle's results):
seed 31 at N = 10, C = 2 gives every agent statuses (4, 0) within 3 + 9 iterations, on the 32-agent K = 3 + 8 batch and
the 8-agent K = 3 + 0 batch; QP alone at most 6 iterations; at tol_qp = 0 statuses (0, 0) and at most 6 QP iterations;
with qp_init = 0 (4, 0) and at most 5 QP iterations; seed 41 at N = 11 and N = 12, 32 agents, (4, 0) within 3 + 8, and
both unchanged in status and counts under the relative 1e-12 input perturbation of tests/shift_cases.py.

A QP-stage factor failure (qp_flag = 1, the body's one `continue`) is not reachable through finite public inputs:
the QP stage factors with iSWIFT's dynamic regularisation (csrc/srb_gj.h: a pivot <= 1e-14 is replaced by 1e-7), so
only a NaN pivot fails there.  No test contrives one.
"""
import numpy as np
import pytest

import moving_oracle
import oracle
import shift_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402

NLP_TOL = 1e-4
POLISHED_TOL = 1e-6
OUT_KEYS = ("x", "x_qp", "obj", "status", "iters", "sel")

CASES = {
    # name: N, C, K_obs, K_nbr, agents, waves asked for (0 automatic), waves expected, seed
    "c11": (10, 2, 3, 8, 32, 1, 1, 31),       # 12_4_1_10_2_11: one wave an agent, four slot trips
    "w4": (10, 2, 3, 0, 8, 0, 4, 31),         # 12_1_4_10_2_3: four waves an agent, one slot trip
    "n11": (11, 2, 3, 8, 32, 1, 1, 41),       # 12_4_1_0_0_0: nz = 12 = NZL, 252 slots in 4 x 64 (run time, one loop)
    "n12": (12, 2, 3, 8, 32, 1, 1, 41),       # 24_5_1_0_0_0: nz = 13 > 12, 275 slots > 256 (run time, NZL 24, one loop)
}
COMPILED = ["c11", "w4"]
# the instance each case launches, asserted through BatchSolver.last_kernels() beside the waves
INSTANCE = {"c11": "12_4_1_10_2_11", "w4": "12_1_4_10_2_3", "n11": "12_4_1_0_0_0", "n12": "24_5_1_0_0_0"}

_cache = {}


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def batch(name, seed=None):
    N, C, Ko, Kn, A = CASES[name][:5]
    seed = CASES[name][7] if seed is None else seed
    if ("b", name, seed) not in _cache:
        b = workload.make_batch(A, N, C, seed=seed)
        for v in b.values():
            v.setflags(write=False)
        _cache[("b", name, seed)] = b
    return _cache[("b", name, seed)]


def oracle_params(name, **kw):
    N, C, Ko, Kn = CASES[name][:4]
    return oracle.params(N, C, K_obs=Ko, K_nbr=Kn, **kw)


def reference(name, **kw):
    """The oracle's solve of the case's batch under oracle.params(**kw), computed once and shared (read only)."""
    key = ("r", name, tuple(sorted(kw.items())))
    if key not in _cache:
        b = batch(name)
        r = oracle.solve_batch(oracle_params(name, **kw), b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"],
                               nthreads=8)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def solver(name, use_nlp=1):
    N, C, Ko, Kn, A, waves = CASES[name][:6]
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), A)
    s.set_waves(waves)
    return s


def solve(s, b, rows=slice(None), **kw):
    out = s.solve(b["x0"][rows], b["ref"][rows], b["foot"][rows], b["obstacles"], b["nbr_state"], **kw)
    return {k: np.array(v, copy=True) for k, v in out.items() if v is not None}


def gpu_solve(name, use_nlp=1, qp_init=None, **options):
    s = solver(name, use_nlp)
    try:
        if qp_init is not None:
            s.set_qp_init(qp_init)
        for k, v in options.items():
            s.set_option(k, v)
        out = solve(s, batch(name), qp_only=not use_nlp)
        assert s.waves() == CASES[name][6]
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE[name], ""), s.last_kernels()
    finally:
        s.close()
    return out


def check_parity(N, out, r, nlp=True):
    cols = slice(0, 2) if nlp else slice(0, 1)
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    print("max |x - oracle| per agent:", e.max(), "statuses", np.unique(out["status"][:, cols], return_counts=True),
          "agents with other counts", int((out["iters"][:, cols] != r["iters"][:, cols]).any(1).sum()),
          "largest count difference", int(np.abs(out["iters"][:, cols] - r["iters"][:, cols]).max()))
    np.testing.assert_array_equal(out["status"][:, cols], r["status"][:, cols])
    np.testing.assert_array_equal(out["iters"][:, cols], r["iters"][:, cols])
    assert e.max() < NLP_TOL, (int(np.argmax(e)), float(e.max()))
    if nlp:
        both = (out["status"][:, 1] == 0) & (r["status"][:, 1] == 0)
        assert both.any()
        assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))
    else:
        eq = np.abs(xus(N, out["x_qp"]) - xus(N, r["x_qp"])).max()
        print("max |x_qp - oracle|:", eq)
        assert eq < POLISHED_TOL


def oracle_ends(r, status, qp_max, nlp_max=None):
    """The oracle fact a case rests on: every agent ends with `status`, within the iteration bounds."""
    st = np.asarray(status)
    assert (r["status"][:, :st.size] == st).all(), np.unique(r["status"], axis=0)
    assert r["iters"][:, 0].max() <= qp_max, r["iters"][:, 0].max()
    if nlp_max is not None:
        assert r["iters"][:, 1].max() <= nlp_max, r["iters"][:, 1].max()


# ---------------------------------------------------------------------------- both compiled instances
@pytest.mark.parametrize("name", COMPILED)
def test_both_stage_bodies_default_options(name):
    r = reference(name)
    oracle_ends(r, (4, 0), 3, 9)
    check_parity(CASES[name][0], gpu_solve(name), r)


@pytest.mark.parametrize("name", COMPILED)
def test_qp_body_alone(name):
    """use_nlp = 0: the QP copy runs, the NLP copy does not; the QP runs to the full tolerance and ends OPTIMAL."""
    r = reference(name, use_nlp=0)
    oracle_ends(r, (0,), 6)
    out = gpu_solve(name, use_nlp=0)
    assert (out["status"][:, 0] == 0).all()
    check_parity(CASES[name][0], out, r, nlp=False)


@pytest.mark.parametrize("name", COMPILED)
def test_stage_hand_off_at_the_full_qp_tolerance(name):
    """qp_warm_tol = 0: the QP copy iterates to 1e-6 and hands that point to the NLP copy (oracle tol_qp = 0)."""
    r = reference(name, tol_qp=0.0)
    oracle_ends(r, (0, 0), 6)
    check_parity(CASES[name][0], gpu_solve(name, qp_warm_tol=0.0), r)


@pytest.mark.parametrize("name", COMPILED)
def test_the_other_qp_start(name):
    """qp_init = 0, iSWIFT's kkt_initialize: the set-up's run-time branch inside the QP copy."""
    r = reference(name, qp_init=0)
    oracle_ends(r, (4, 0), 5)
    check_parity(CASES[name][0], gpu_solve(name, qp_init=0), r)


# ---------------------------------------------------------------------------- what follows the NLP copy
def test_polish_after_the_split_body():
    """polish_fused 0 against 1 on the 32-agent batch: the separate polish kernel starts from what the NLP copy
    exported, the fused one from what it left in LDS and registers (tests/test_gpu_parity.py
    test_fused_polish_equals_separate_polish_kernel: statuses identical, x within 1e-8)."""
    s = solver("c11")
    try:
        fu = solve(s, batch("c11"))
        assert s.get_option("last_polish") == 2.0
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE["c11"], "")
        s.set_option("polish_fused", 0)
        se = solve(s, batch("c11"))
        assert s.get_option("last_polish") == 1.0
        assert s.waves() == 1
        # (polish_waves at its default: the one-wave solve is polished by the two-wave instance of the same NZL)
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE["c11"], "srb_polish_kernel_12_2_2_0_0_0")
    finally:
        s.close()
    print("max |x fused - x kernel|:", np.abs(fu["x"] - se["x"]).max())
    np.testing.assert_array_equal(fu["status"], se["status"])
    np.testing.assert_allclose(fu["x"], se["x"], atol=1e-8, rtol=0)


@pytest.mark.parametrize("name", COMPILED)
def test_nothing_leaks_across_stages_or_solves(name):
    """One context: batch A (seed 31), batch B (seed 32), A again -- the first and third results equal in every array."""
    s = solver(name)
    try:
        a1 = solve(s, batch(name))
        b1 = solve(s, batch(name, seed=32))
        a2 = solve(s, batch(name))
        assert s.waves() == CASES[name][6]
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE[name], "")
    finally:
        s.close()
    assert set(a1) == set(a2)
    assert not np.array_equal(a1["x"], b1["x"])
    for k in a1:
        assert np.array_equal(a1[k], a2[k], equal_nan=True), k


def test_a_shard_equals_its_rows_of_the_whole_batch():
    """Agents 16 .. 31 of the 32-agent batch as a shard (agent_offset 16, the whole neighbour snapshot and obstacle
    table, one wave an agent as the whole batch): bit for bit the same rows."""
    s = solver("c11")
    try:
        whole = solve(s, batch("c11"))
        part = solve(s, batch("c11"), rows=slice(16, 32), agent_offset=16)
        assert s.waves() == 1
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE["c11"], "")
    finally:
        s.close()
    for k in OUT_KEYS:
        assert np.array_equal(whole[k][16:32], part[k], equal_nan=True), k


# ---------------------------------------------------------------------------- the mv form
def test_moving_obstacle_form():
    """srb_nmpc_kernel_mv_12_4_1_10_2_11: the 32-agent batch with a velocity table, against moving_oracle.solve (the
    numpy restatement) at the bounds of tests/test_moving_obstacles.py assert_matches."""
    N, C, Ko, Kn, A = CASES["c11"][:5]
    b = batch("c11")
    vel = workload.obstacle_velocities(b["obstacles"].shape[0], 31, 1.0)
    r = moving_oracle.solve(oracle_params("c11"), b, vel)
    r0 = reference("c11")
    assert (np.abs(r["x"][:, :6 * N] - r0["x"][:, :6 * N]).max(1) > 1e-3).sum() >= 4          # the table matters
    s = solver("c11")
    try:
        out = solve(s, b, obs_vel=vel)
        assert s.waves() == 1
        assert s.last_kernels() == ("srb_nmpc_kernel_mv_" + INSTANCE["c11"], "")
    finally:
        s.close()
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max()
    print(f"max |X,U,s - oracle| = {e:.3e}, iterations equal on {np.mean(np.all(out['iters'] == r['iters'], 1)):.3f}")
    np.testing.assert_array_equal(out["status"], r["status"])
    assert np.mean(np.all(out["iters"] == r["iters"], 1)) >= 0.85
    assert np.abs(out["iters"] - r["iters"]).max() <= 2
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)
    np.testing.assert_allclose(out["x"], r["x"], atol=NLP_TOL, rtol=0)
    np.testing.assert_allclose(out["obj"], r["obj"], rtol=1e-7, atol=1e-6)
    assert np.array_equal(out["sel"], r["sel"])


# ---------------------------------------------------------------------------- the instances that broke last time
@pytest.mark.parametrize("name", ["n11", "n12"])
def test_run_time_instances_keep_their_results(name):
    """N = 11 launches 12_4_1_0_0_0 and N = 12 launches 24_5_1_0_0_0 (the first fitting entries of
    SRB_KERNEL_INSTANCES for nz = N + 1 and (6 + C) N + 1 + 2 (N - 1) + 2 N + 11 N slots at 64 lanes): the one loop,
    whose machine code the split leaves as it was.  The oracle's statuses and counts on these batches do not move
    under the 1e-12 probe, so the kernel is held to them exactly."""
    N, C, Ko, Kn, A = CASES[name][:5]
    nz, slots = N * (C - 1) + 1, (6 + C) * N + 1 + 2 * (N - 1) + 2 * N + N * (Ko + Kn)
    assert (nz, slots) == {"n11": (12, 252), "n12": (13, 275)}[name]
    b, r = batch(name), reference(name)
    oracle_ends(r, (4, 0), 3, 8)
    p = oracle_params(name)
    for bp in shift_cases.perturbed(b, ("x0", "ref", "foot")):
        q = oracle.solve_batch(p, bp["x0"], bp["ref"], bp["foot"], bp["obstacles"], bp["nbr_state"], nthreads=8)
        np.testing.assert_array_equal(q["status"], r["status"])
        np.testing.assert_array_equal(q["iters"], r["iters"])
    check_parity(N, gpu_solve(name), r)
