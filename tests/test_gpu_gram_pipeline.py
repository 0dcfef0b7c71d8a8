"""GPU tests of the pipelined Gram of the solve kernel (csrc/srb_kernels.hip gram_rhs, rhs_only, UlLane).  In the
instances with one column block (NZL <= 16) the operand loads of batch b + 1 are issued before the MFMAs of batch
b, the first batch is loaded ahead of the loop and the last one peeled, the obstacle range starts its loads under
the last batch of the row range, and the `a` loads are unconditional (column clamped into the row, zero selected
for the padding columns); at one wave per agent the U / lambda / slack sums of ul_add are formed by the lane that
holds the entry and stored with it.  The shapes are the smallest at which a look-ahead load or the lane mapping
can go wrong (SHAPES, one line each); the N = 20 instance (two column blocks) keeps the one-batch-at-a-time loop
and runs as the control of the shared helpers.

Comparison rule, as tests/test_gpu_slot_kinds.py: statuses equal, iteration counts equal, X, U, s within 1e-4,
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
    # 16 term rows: one row batch, the peeled last batch is also the first; 33 obstacle rows: an odd number of
    # obstacle batches, the last one padded
    "n3": (3, 2, 3, 8, 32, 1, 1),
    # 22 term rows, 44 obstacle rows: two row batches, the second mostly padding
    "n4": (4, 2, 3, 8, 32, 1, 1),
    # nz = 12 = NZL: no padding column (the clamp is never the select); 64 term rows, 121 obstacle rows: eight batches
    "n11": (11, 2, 3, 8, 32, 1, 1),
    # 10 obstacle rows: exactly one obstacle batch after four row batches
    "k1": (10, 2, 1, 0, 32, 1, 1),
    # NZL 16, C = 4: the U / lambda rows with 9 entries a grid and 6 rows
    "c4": (5, 4, 3, 8, 32, 1, 1),
    # the compiled default instance 12_4_1_10_2_11
    "default": (10, 2, 3, 8, 64, 1, 1),
    # 12_1_4_10_2_3: one batch per wave in both ranges, the `part` path; no prefetch may leave a wave's chunk
    "w4": (10, 2, 3, 0, 8, 0, 4),
    # 24_4_2: NZM = 32, interleaved FULL / non-FULL batches, the folded obstacle range, wave 1 adding in place
    "n20": (20, 2, 3, 8, 16, 2, 2),
    # crowded(16, 10, seed=5): active obstacle rows with large weights; agents leave the loop through the FATAL /
    # ACCEPTABLE breaks between a Gram and its use
    "crowded": (10, 2, 3, 8, 16, 1, 1),
}

# the instance each case launches, asserted through BatchSolver.last_kernels() beside the waves
INSTANCE = {"n3": "12_3_1_0_0_0", "n4": "12_3_1_0_0_0", "n11": "12_4_1_0_0_0", "k1": "12_3_1_0_0_0", "c4": "16_4_1_0_0_0",
            "default": "12_4_1_10_2_11", "w4": "12_1_4_10_2_3", "n20": "24_4_2_20_2_11", "crowded": "12_4_1_10_2_11"}
# the polish kernel of polish_fused = 0 at the default polish_waves: a one-wave solve is polished at two waves, by the
# first two-wave instance of the same NZL
POLISH_KERNEL = {"default": "srb_polish_kernel_12_2_2_0_0_0", "n3": "srb_polish_kernel_12_2_2_0_0_0"}

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


def gpu_solve(name, fused=1, use_nlp=1, solves=1):
    N, C, Ko, Kn, A, waves, want = SHAPES[name]
    b = batch(name)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), A)
    try:
        s.set_waves(waves)
        s.set_option("polish_fused", fused)
        outs = []
        for _ in range(solves):
            out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], qp_only=not use_nlp)
            outs.append({k: np.array(v, copy=True) for k, v in out.items() if v is not None})
        assert s.waves() == want
        polish = POLISH_KERNEL[name] if use_nlp and not fused else ""
        assert s.last_kernels() == ("srb_nmpc_kernel_" + INSTANCE[name], polish), s.last_kernels()
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
def test_pipelined_passes_match_oracle(name):
    check_parity(SHAPES[name][0], gpu_solve(name), reference(name))


@pytest.mark.parametrize("name", ["default", "n3"])
def test_polish_kernel_gram(name):
    """polish_fused = 0: the polish runs in srb_polish_kernel, whose own gram_rhs / rhs_only are the pipelined ones
    (polish_fused = 1, the fused polish, is the case above)."""
    check_parity(SHAPES[name][0], gpu_solve(name, fused=0), reference(name))


@pytest.mark.parametrize("name", ["default", "n3"])
def test_qp_only_touches_no_obstacle_range(name):
    """use_nlp = 0: every Gram runs with nko = 0, the row range alone (its last batch peeled with nothing after it)."""
    check_parity(SHAPES[name][0], gpu_solve(name, use_nlp=0), reference(name, use_nlp=0), nlp=False)


def test_two_solves_on_one_context_are_bit_equal():
    """The compiled default instance, 64 agents, solved twice on one context: every output array equal bit for bit
    (a stale prefetch buffer would show here first)."""
    o1, o2 = gpu_solve("default", solves=2)
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
