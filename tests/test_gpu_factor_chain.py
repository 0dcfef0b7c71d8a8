"""GPU tests of the solve kernel's factor chain (csrc/srb_gj.h gj_factor, csrc/srb_kernels.hip nmpc_agent): the
reduced Newton matrix is inverted by the DPP row_newbcast Gauss-Jordan where its rows are replicated in every
16-lane row of the wave (NZL <= 16) and by the readlane form otherwise, and the first inertia shift is formed only
when a factorisation fails.  The shapes are the smallest at which the elimination's column order, its identity
padding or the uniform failure branch can go wrong (SHAPES, one line each).

Comparison rule, as tests/test_gpu_gram_pipeline.py: statuses equal, iteration counts equal, X, U, s within 1e-4,
within 1e-6 where both sides end NLP OPTIMAL.
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


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def crowded(A, N, C, seed):
    """tests/test_gpu_slot_kinds.py `crowded`: four times the reference's obstacle density."""
    return workload.make_batch(A, N, C, seed=seed, n_obs=int(round(80 * workload.arena_scale(A) ** 2)))


SHAPES = {
    # name: N, C, K_obs, K_nbr, agents, waves asked for (0 automatic), waves expected
    # nz = 3, the smallest horizon the library accepts (srb_ctx_create: N >= 2; N = 1, nz = 2, is refused, see
    # test_horizon_one_is_refused): the (k + 1 + jj) % NZE column order wraps after one column; 45 slots fit one trip, so
    # this is 8_1_1 (NZL 8), five padded steps -- no N = 2 shape reaches an NZL 12 instance
    "n2": (2, 2, 3, 8, 32, 1, 1),
    # nz = 4 in NZL 12 at run time, NZE = NZL: identity steps after the last real pivot
    "n3": (3, 2, 3, 8, 32, 1, 1),
    # nz = 12 = NZL: no padding step
    "n11": (11, 2, 3, 8, 32, 1, 1),
    # NZL 16, C = 4: the widest one-block row
    "c4": (5, 4, 3, 8, 32, 1, 1),
    # the compiled default instance 12_4_1_10_2_11: NZE = 11, both stages
    "default": (10, 2, 3, 8, 64, 1, 1),
    # 12_1_4_10_2_3, four waves: every wave factors redundantly; the failure branch stays uniform over the workgroup
    "w4": (10, 2, 3, 0, 8, 0, 4),
    # 24_4_2_20_2_11, NZL 24: rows not replicated (the readlane form), the LEAN body, the folded obstacle range
    "n20": (20, 2, 3, 8, 16, 2, 2),
    # crowded(16, 10, 2, seed=5): agents leave the loop through the FATAL / ACCEPTABLE breaks between a factor and its use
    "crowded": (10, 2, 3, 8, 16, 1, 1),
}

# the instance each case launches, asserted through BatchSolver.last_kernels() beside the waves
INSTANCE = {"n2": "8_1_1_0_0_0", "n3": "12_3_1_0_0_0", "n11": "12_4_1_0_0_0", "c4": "16_4_1_0_0_0", "default": "12_4_1_10_2_11",
            "w4": "12_1_4_10_2_3", "n20": "24_4_2_20_2_11", "crowded": "12_4_1_10_2_11"}

_cache = {}


def batch(name):
    if ("b", name) not in _cache:
        N, C, Ko, Kn, A, _, _ = SHAPES[name]
        _cache[("b", name)] = crowded(A, N, C, seed=5) if name == "crowded" else workload.make_batch(A, N, C, seed=17 * N + C + Kn)
    return _cache[("b", name)]


def reference(name, use_nlp=1):
    """The oracle's solve of the case's batch, computed once and shared."""
    if ("r", name, use_nlp) not in _cache:
        N, C, Ko, Kn = SHAPES[name][:4]
        b = batch(name)
        _cache[("r", name, use_nlp)] = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), b["x0"],
                                                         b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nthreads=8)
    return _cache[("r", name, use_nlp)]


def gpu_solve(name, use_nlp=1, solves=1):
    N, C, Ko, Kn, A, waves, want = SHAPES[name]
    b = batch(name)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), A)
    try:
        s.set_waves(waves)
        outs = []
        for _ in range(solves):
            out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], qp_only=not use_nlp)
            outs.append({k: np.array(v, copy=True) for k, v in out.items() if v is not None})
        assert s.waves() == want
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE[name], ""), s.last_kernels()
    finally:
        s.close()
    return outs if solves > 1 else outs[0]


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
        assert np.abs(xus(N, out["x_qp"]) - xus(N, r["x_qp"])).max() < POLISHED_TOL


@pytest.mark.parametrize("name", list(SHAPES))
def test_factor_chain_matches_oracle(name):
    check_parity(SHAPES[name][0], gpu_solve(name), reference(name))


@pytest.mark.parametrize("name", ["n3", "default"])
def test_qp_only_factors_with_regularisation(name):
    """use_nlp = 0: the regularise = 1 factorisations only; the QP stage never forms a shift."""
    check_parity(SHAPES[name][0], gpu_solve(name, use_nlp=0), reference(name, use_nlp=0), nlp=False)


def test_horizon_one_is_refused():
    """N = 1 (nz = 2) is outside the library's contract: the context is refused, no kernel runs.  The n2 case above
    is the smallest elimination a solve can reach."""
    with pytest.raises(RuntimeError, match="N >= 2"):
        srbnmpc.BatchSolver(srbnmpc.default_params(1, 2, K_obs=3, K_nbr=8), 32)


def test_two_solves_on_one_context_are_bit_equal():
    """The compiled default instance, 64 agents, solved twice on one context: every output array equal bit for bit."""
    o1, o2 = gpu_solve("default", solves=2)
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
