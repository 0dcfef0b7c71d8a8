"""GPU tests of the vector-ALU reduced Gram of the solve kernel (csrc/srb_gram.h gram_rhs, SRB_GRAM_DPP_ASM): in the
compiled one-wave, one-column-block instance (12_4_1_10_2_11 and its f32 / mv forms, their polish kernels) lane
(kq, li) accumulates column li of H over the term rows of its row kq with v_fmac_f64_dpp row_newbcast, the batch
sequence unrolled and the accumulators above a group's highest non-zero column left out; a reduce-scatter by permlane
swaps then puts H[kq + 4q][li] where the MFMA's D layout had it.  The run-time instances (12_4_1, 12_3_1, 8_1_1) keep
the MFMA form -- the vector form put 12_4_1 and 12_3_1 deeper into scratch -- and run here as the cases that share
gram_rhs's loads, UlLane sums and stores with it: a batch that is almost all padding, one row batch, a peeled batch
that is also the first, no idle column.

Comparison rule, as tests/test_gpu_gram_pipeline.py: statuses and iteration counts equal to the oracle's, X, U, s
within 1e-4, within 1e-6 where both sides end NLP OPTIMAL.
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

SHAPES = {
    # name: N, C, K_obs, K_nbr, agents; one wave an agent asked for and expected in every case
    "n2": (2, 2, 3, 8, 32),         # nz = 3: most columns and lanes idle, one row batch, 22 obstacle rows in two batches
    "n2k1": (2, 2, 1, 0, 32),       # 2 obstacle rows: a batch that is almost all padding
    "n3": (3, 2, 3, 8, 32),         # the peeled last batch is also the first
    "n4": (4, 2, 3, 8, 32),         # the second row batch is mostly padding
    "n11": (11, 2, 3, 8, 32),       # nz = 12 = NZL: no idle column
    "k1": (10, 2, 1, 0, 32),        # exactly one obstacle batch
    "default": (10, 2, 3, 8, 64),   # the compiled instance 12_4_1_10_2_11: the vector form
    "crowded": (10, 2, 3, 8, 16),   # crowded(16, 10, 2, seed=5): large active weights; exits between a Gram and its use
}
# the instance each case launches at one wave an agent, asserted through BatchSolver.last_kernels()
INSTANCE = {"n2": "8_1_1_0_0_0", "n2k1": "8_1_1_0_0_0", "n3": "12_3_1_0_0_0", "n4": "12_3_1_0_0_0", "n11": "12_4_1_0_0_0",
            "k1": "12_3_1_0_0_0", "default": "12_4_1_10_2_11", "crowded": "12_4_1_10_2_11"}
# every agent of these ends QP OPTIMAL (warm tolerance: status 4) / NLP OPTIMAL on the oracle, so the rule's
# "both OPTIMAL" set is the whole batch
ALL_OPTIMAL = ["n2", "n2k1", "n3", "n11", "k1"]

_cache = {}


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def batch(name):
    if ("b", name) not in _cache:
        N, C, Ko, Kn, A = SHAPES[name]
        if name == "crowded":       # tests/test_gpu_gram_pipeline.py `crowded`: four times the reference's obstacle density
            b = workload.make_batch(A, N, C, seed=5, n_obs=int(round(80 * workload.arena_scale(A) ** 2)))
        else:
            b = workload.make_batch(A, N, C, seed=17 * N + C + Kn)
        for v in b.values():
            v.setflags(write=False)
        _cache[("b", name)] = b
    return _cache[("b", name)]


def oracle_solve(name, b, use_nlp=1):
    N, C, Ko, Kn = SHAPES[name][:4]
    return oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), b["x0"], b["ref"], b["foot"],
                              b["obstacles"], b["nbr_state"], nthreads=8)


def reference(name, use_nlp=1):
    """The oracle's solve of the case's batch, computed once and shared (read only)."""
    if ("r", name, use_nlp) not in _cache:
        r = oracle_solve(name, batch(name), use_nlp)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[("r", name, use_nlp)] = r
    return _cache[("r", name, use_nlp)]


def gpu_solve(name, use_nlp=1, solves=1, options=None, want_option=None, form="", polish="", **kw):
    """form: the infix of the solve kernel expected ("", "f32_", "mv_"); polish: the polish kernel expected, as
    "<prefix><instance>" ("" where the polish runs fused or not at all)."""
    N, C, Ko, Kn, A = SHAPES[name]
    b = batch(name)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=use_nlp), A)
    try:
        s.set_waves(1)
        for k, v in (options or {}).items():
            s.set_option(k, v)
        outs = []
        for _ in range(solves):
            out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], qp_only=not use_nlp, **kw)
            outs.append({k: np.array(v, copy=True) for k, v in out.items() if v is not None})
        assert s.waves() == 1                   # no case may silently run another instance family
        assert s.last_kernels() == ("srb_nmpc_kernel_" + form + INSTANCE[name], polish), s.last_kernels()
        for k, v in (want_option or {}).items():
            assert s.get_option(k) == v, (k, s.get_option(k))
    finally:
        s.close()
    return outs if solves > 1 else outs[0]


def check_parity(N, out, r, nlp=True, all_optimal=False):
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
        assert both.all() if all_optimal else both.any()
        assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))
    else:
        eq = np.abs(xus(N, out["x_qp"]) - xus(N, r["x_qp"])).max()
        print("max |x_qp - oracle|:", eq)
        assert eq < POLISHED_TOL


@pytest.mark.parametrize("name", list(SHAPES))
def test_gram_matches_oracle(name):
    r = reference(name)
    if name in ALL_OPTIMAL:
        assert (r["status"][:, 1] == 0).all() and np.isin(r["status"][:, 0], (0, 4)).all(), np.unique(r["status"], axis=0)
    check_parity(SHAPES[name][0], gpu_solve(name), r, all_optimal=name in ALL_OPTIMAL)


@pytest.mark.parametrize("name", ["n2", "n2k1"])
def test_smallest_cases_are_insensitive_on_the_oracle(name):
    """What holds n2 and n2k1 to the oracle's counts exactly: three random relative 1e-12 perturbations of the inputs
    (tests/shift_cases.py) move no status and no count there."""
    r = reference(name)
    for bp in shift_cases.perturbed(batch(name), ("x0", "ref", "foot")):
        q = oracle_solve(name, bp)
        np.testing.assert_array_equal(q["status"], r["status"])
        np.testing.assert_array_equal(q["iters"], r["iters"])


@pytest.mark.parametrize("name", ["n2", "default"])
def test_qp_only_touches_no_obstacle_range(name):
    """use_nlp = 0: every Gram runs with nko = 0, the row batches alone (in the vector form the unrolled sequence ends
    after them, the UlLane loads under the last row batch)."""
    r = reference(name, use_nlp=0)
    assert (r["status"][:, 0] == 0).all()
    check_parity(SHAPES[name][0], gpu_solve(name, use_nlp=0), r, nlp=False)


@pytest.mark.parametrize("polish_waves,kernel", [(1, "srb_polish_kernel_12_4_1_10_2_11"), (0, "srb_polish_kernel_12_2_2_0_0_0")])
def test_polish_kernel_gram(polish_waves, kernel):
    """polish_fused = 0 with polish_waves = 1: the polish runs in srb_polish_kernel_12_4_1_10_2_11, whose own Gram is the
    vector one.  At the default polish_waves = 0 a one-wave solve is polished at two waves, by the first two-wave
    instance of the same NZL: srb_polish_kernel_12_2_2_0_0_0, whose Gram is the MFMA one."""
    out = gpu_solve("default", options={"polish_fused": 0, "polish_waves": polish_waves}, want_option={"last_polish": 1.0},
                    polish=kernel)
    check_parity(SHAPES["default"][0], out, reference("default"))


def test_fp32_factor_form():
    """kkt_fp32_mu = 0.1: srb_nmpc_kernel_f32_12_4_1_10_2_11 (the reduced matrix inverted in fp32 above the threshold,
    every solve refined in fp64 against the fp64 H this Gram forms), by the same rule."""
    out = gpu_solve("default", options={"kkt_fp32_mu": 0.1}, want_option={"last_kkt_fp32": 1.0}, form="f32_")
    check_parity(SHAPES["default"][0], out, reference("default"))


def test_moving_obstacle_form():
    """srb_nmpc_kernel_mv_12_4_1_10_2_11 with a zero-velocity table: the table instance computes what the plain one
    does (tests/test_moving_obstacles.py: moving_oracle.solve with zero velocities is the oracle's solve), so the rule
    holds against the shared reference; moving_oracle.solve itself at that test's bounds beside it."""
    N = SHAPES["default"][0]
    b, r = batch("default"), reference("default")
    vel = np.zeros((b["obstacles"].shape[0], 2))
    out = gpu_solve("default", form="mv_", obs_vel=vel)
    check_parity(N, out, r)
    Ko, Kn = SHAPES["default"][2:4]
    m = moving_oracle.solve(oracle.params(N, 2, K_obs=Ko, K_nbr=Kn), b, vel)
    np.testing.assert_array_equal(out["status"], m["status"])
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, m["x"]), atol=NLP_TOL, rtol=0)


def test_two_solves_on_one_context_are_bit_equal():
    """n11 solved twice on one context: every output array equal bit for bit."""
    o1, o2 = gpu_solve("n11", solves=2)
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k


def test_two_solves_of_the_vector_form_are_bit_equal():
    """The same for the compiled instance, whose accumulators and look-ahead buffers are the new ones."""
    o1, o2 = gpu_solve("default", solves=2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
