"""GPU tests of the staged LDS loads of the solve kernel (row_dot, the la_solve refinement row, obs_relin):
the helpers now read a whole term row into registers before the first use, so the shapes here are the
smallest at which such a staged read can go wrong -- rows far shorter than the register bound, a full row
with no padding column, the NZL 16 instance with the C = 4 basis, the compiled default instance, the
four-wave instance (no staged value may cross a barrier), the folded N = 20 path, and a crowded arena whose
agents leave the iteration loop through its FATAL and ACCEPTABLE breaks.

Each case compares with the oracle exactly as tests/test_gpu_parity.py::test_gpu_matches_oracle does: statuses
equal, iteration counts equal but for round-off at an exit threshold, X, U, s within that test's bounds.
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

QP_TOL = 1e-6       # as tests/test_gpu_parity.py
NLP_TOL = 1e-4


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def check_vs_oracle(N, C, Ko, Kn, b, waves, want_waves, instance):
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=1), b["x0"].shape[0])
    try:
        s.set_waves(waves)
        out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
        assert s.waves() == want_waves
        assert s.last_kernels() == ("srb_nmpc_kernel_" + instance, ""), s.last_kernels()
    finally:
        s.close()
    r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=1), b["x0"], b["ref"], b["foot"],
                           b["obstacles"], b["nbr_state"], nthreads=8)
    bad = np.where((out["status"] != r["status"]).any(1))[0]
    assert bad.size == 0, [(int(a), out["status"][a].tolist(), r["status"][a].tolist(), out["iters"][a].tolist(),
                            r["iters"][a].tolist()) for a in bad]
    assert np.mean(np.all(out["iters"] == r["iters"], 1)) >= 0.85
    assert np.abs(out["iters"] - r["iters"]).max() <= 2
    np.testing.assert_allclose(xus(N, out["x_qp"]), xus(N, r["x_qp"]), atol=QP_TOL, rtol=0)
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)
    if C == 2:
        np.testing.assert_allclose(out["x"], r["x"], atol=NLP_TOL, rtol=0)
    np.testing.assert_allclose(out["obj"], r["obj"], rtol=1e-7, atol=1e-6)
    return out, r


SHAPES = [
    # N, C, K_obs, K_nbr, agents, waves asked for (0 automatic), waves expected
    (3, 2, 3, 8, 32, 1, 1),      # nz = 4 in the run-time NZL 12 instance: rows far shorter than NZL, identity padding
    (11, 2, 3, 8, 32, 1, 1),     # nz = 12 = NZL, run-time instance: even row length, a full row, no padding column
    (5, 4, 3, 8, 32, 1, 1),      # nz = 16: the NZL 16 instance and the C = 4 basis
    (10, 2, 3, 8, 64, 1, 1),     # the compiled default instance 12_4_1_10_2_11 itself
    (10, 2, 3, 0, 8, 0, 4),      # four waves per agent (the compiled 12_1_4): the staging must not cross a barrier
    (20, 2, 3, 8, 16, 2, 2),     # the compiled 24_4_2: the folded obstacle path, LEAN
]


# the instance each shape launches, by (N, C, K_obs + K_nbr, waves): asserted through BatchSolver.last_kernels()
INSTANCE = {(3, 2, 11, 1): "12_3_1_0_0_0", (11, 2, 11, 1): "12_4_1_0_0_0", (5, 4, 11, 1): "16_4_1_0_0_0",
            (10, 2, 11, 1): "12_4_1_10_2_11", (10, 2, 3, 4): "12_1_4_10_2_3", (20, 2, 11, 2): "24_4_2_20_2_11"}


@pytest.mark.parametrize("N,C,Ko,Kn,A,waves,want", SHAPES)
def test_staged_loads_match_oracle(N, C, Ko, Kn, A, waves, want):
    b = workload.make_batch(A, N, C, seed=11 * N + C + Kn)
    check_vs_oracle(N, C, Ko, Kn, b, waves, want, INSTANCE[(N, C, Ko + Kn, want)])


def test_crowded_arena_break_paths_match_oracle():
    """The crowded arena of test_qp_warm_tolerance_leaves_the_nlp_result's `dense` case (four times the
    reference's obstacle density): some agents end FATAL or ACCEPTABLE, leaving the iteration loop after staged
    stores; they must return the oracle's point and status.  (Seed 5 on the CPU oracle: non-OPTIMAL agents
    present, asserted below.)"""
    N, C, Ko, Kn = 10, 2, 3, 8
    b = workload.make_batch(1024, N, C, seed=5, n_obs=int(round(80 * workload.arena_scale(1024) ** 2)))
    out, r = check_vs_oracle(N, C, Ko, Kn, b, 0, 1, "12_4_1_10_2_11")
    assert (r["status"][:, 1] != 0).any(), "the workload must drive some agents off the OPTIMAL exit"
    np.testing.assert_array_equal(out["status"], r["status"])
