"""The compiled-shape solve / polish kernels specialise every slot pass by the kinds a slot trip can hold
(csrc/srb_kernel_params.h srb_trip_kinds, csrc/srb_kernels.hip SlotTrips): single-row obstacle trips carry no
row 1, all-VAR trips no masks, and the per-grid obstacle-dual sum is formed once an iteration.  These runs put the
specialised trips to work on small batches -- active obstacle rows with non-zero duals, the fused polish and the
polish kernel, the QP-only two-trip path, tables so small that most selected rows are the -1 / 1000 m rows, the
N = 20 instance at two waves, and the run-time instance as the control -- against the oracle, with the parity rule
of tests/test_gpu_parity.py made exact in the counts:

  statuses and iteration counts equal; X, U, s within 1e-4; within 1e-6 where both sides polished (NLP OPTIMAL).
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402

NLP_TOL = 1e-4
POLISHED_TOL = 1e-6
C = 2
KO = 3


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def crowded(A, N, seed):
    """A batch in an arena with four times the reference's obstacle density (tests/test_gpu_parity.py "dense")."""
    return workload.make_batch(A, N, C, seed=seed, n_obs=int(round(80 * workload.arena_scale(A) ** 2)))


_cache = {}


def batch16():
    if "b16" not in _cache:
        _cache["b16"] = crowded(16, 10, seed=5)
    return _cache["b16"]


def reference(key, N, Kn, b, use_nlp=1):
    """The oracle's solve of batch b, computed once per case and shared."""
    if key not in _cache:
        _cache[key] = oracle.solve_batch(oracle.params(N, C, K_obs=KO, K_nbr=Kn, use_nlp=use_nlp), b["x0"], b["ref"],
                                         b["foot"], b["obstacles"], b["nbr_state"], nthreads=8)
    return _cache[key]


def gpu_solve(N, Kn, b, waves, instance, fused=1, use_nlp=1, polish=""):
    """instance: the solve kernel's instance, polish: the polish kernel's name ("": fused or none), both asserted
    through BatchSolver.last_kernels()."""
    A = b["x0"].shape[0]
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=KO, K_nbr=Kn, use_nlp=use_nlp), A)
    try:
        s.set_waves(waves)
        s.set_option("polish_fused", fused)
        out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], qp_only=not use_nlp)
        assert s.waves() == waves
        assert s.last_kernels() == ("srb_nmpc_kernel_" + instance, polish), s.last_kernels()
        out["last_polish"] = s.get_option("last_polish")
    finally:
        s.close()
    return out


def check_parity(N, out, r, nlp=True):
    cols = slice(0, 2) if nlp else slice(0, 1)
    np.testing.assert_array_equal(out["status"][:, cols], r["status"][:, cols])
    np.testing.assert_array_equal(out["iters"][:, cols], r["iters"][:, cols])
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    print("max |x - oracle| per agent:", e.max(), "statuses", np.unique(out["status"][:, cols], return_counts=True))
    assert e.max() < NLP_TOL, (int(np.argmax(e)), float(e.max()))
    if nlp:
        both = (out["status"][:, 1] == 0) & (r["status"][:, 1] == 0)
        assert both.any()
        assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))
    else:
        assert np.abs(xus(N, out["x_qp"]) - xus(N, r["x_qp"])).max() < POLISHED_TOL


def active_obstacle_rows(N, Kn, b, x):
    """Rows d^2 + s - eps of the solution x that sit on their bound (1e-6), over the batch."""
    op = oracle.params(N, C, K_obs=KO, K_nbr=Kn)
    cnt = 0
    for a in range(x.shape[0]):
        obs, eps = oracle.select_obstacles(op, b["x0"][a], b["obstacles"], b["nbr_state"], a)
        p = x[a, :4 * N].reshape(N, 4)[:, [0, 2]]
        d2 = ((p[:, None, :] - obs) ** 2).sum(-1)
        cnt += int((d2 + x[a, -1] - eps[None, :] < 1e-6).sum())
    return cnt


@pytest.mark.parametrize("fused", [1, 0])
def test_compiled_one_wave_instance_with_active_obstacle_rows(fused):
    """16 agents, N = 10, K = 3 + 8 at one wave per agent (12_4_1_10_2_11) in a crowded arena: obstacle rows are
    active, so the single-row trips carry non-zero duals through the iteration, the carried dual sum and the polish
    (fused = 1: at the end of the solve kernel; 0: a polish kernel -- at the default polish_waves the two-wave
    srb_polish_kernel_12_2_2_0_0_0, not the instance's own)."""
    b = batch16()
    r = reference("c16", 10, 8, b)
    assert active_obstacle_rows(10, 8, b, r["x"]) >= 4          # the workload does what it is for
    out = gpu_solve(10, 8, b, 1, "12_4_1_10_2_11", fused=fused, polish="" if fused else "srb_polish_kernel_12_2_2_0_0_0")
    assert out["last_polish"] == (2.0 if fused else 1.0)
    check_parity(10, out, r)


def test_qp_only_two_trip_path():
    """The same batch, QP only (use_nlp = 0): the stage that runs the VAR and the mixed trip alone."""
    b = batch16()
    r = reference("q16", 10, 8, b, use_nlp=0)
    out = gpu_solve(10, 8, b, 1, "12_4_1_10_2_11", use_nlp=0)
    check_parity(10, out, r, nlp=False)


def test_small_tables_leave_sentinel_rows():
    """3 agents and 2 static rows: the tables are padded with NaN rows to the K = 3 + 8 the instance is compiled for
    (a table shorter than K would clamp K and select the run-time instance), so one static column falls back to row
    0 and six of the eight neighbour columns are -1, the 1000 m rows."""
    b = workload.make_batch(3, 10, C, seed=2)
    b["obstacles"] = np.vstack([b["obstacles"][:2], [[np.nan, np.nan]]])
    b["nbr_state"] = np.vstack([b["nbr_state"], np.full((6, 4), np.nan)])
    r = reference("small", 10, 8, b)
    out = gpu_solve(10, 8, b, 1, "12_4_1_10_2_11")
    assert out["sel"].shape == (3, 11) and ((out["sel"][:, KO:] == -1).sum(1) == 6).all(), out["sel"]
    check_parity(10, out, r)


def test_config5_instance_two_waves():
    """8 agents, N = 20 at two waves per agent: 24_4_2_20_2_11 (folded obstacle rows, recomputed reciprocals).  The
    neighbour table is padded with one NaN row, as in test_small_tables_leave_sentinel_rows: eight rows would clamp K_nbr
    to 7 and launch the run-time 24_4_2_0_0_0 (which this test did until it asserted the kernel's name)."""
    b = crowded(8, 20, seed=3)
    b["nbr_state"] = np.vstack([b["nbr_state"], np.full((1, 4), np.nan)])
    r = reference("n20", 20, 8, b)
    out = gpu_solve(20, 8, b, 2, "24_4_2_20_2_11")
    check_parity(20, out, r)


def test_run_time_instance_control():
    """The 16 agents with K_nbr = 7: no compiled shape has K = 10, so the run-time 12_4_1_0_0_0 solves it."""
    b = batch16()
    r = reference("ctl", 10, 7, b)
    out = gpu_solve(10, 7, b, 1, "12_4_1_0_0_0")
    check_parity(10, out, r)
