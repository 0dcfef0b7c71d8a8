"""GPU tests of the corrector's right-hand side from slot-owned rows (csrc/srb_gram.h rhs_slots): in the compiled
one-wave instance 12_4_1_10_2_11 (its f32 / mv forms, its polish kernel, the fused polish) the NLP stage's corrector
pass and polish_stationary keep each slot's coefficient in a register of the lane that owns the slot, add
coefficient x (the slot's term row) to eleven private accumulators and sum the 64 lanes' partials in a fixed order,
instead of storing the coefficients to LDS (the VEL rows' by atomic) and walking the rows in the Gram's layout
(rhs_only, which every other instance keeps -- and the QP stage's copy of this one: SRB_RHS_SLOTS_QP 0, the
microbenchmark's gate failed at the QP size; built with 1 the QP cases below run the form).  g is the same sum in
another association.

The instance exists only at N = 10, C = 2, K = 3 + 8, so every case is that shape at 16 to 64 agents with set_waves(1);
each solve asserts the kernels it launched (BatchSolver.last_kernels()) before anything is compared.

Comparison rule, as tests/test_gpu_gram_valu.py (whose batches and cached oracle solves these cases share): statuses
and iteration counts equal to the oracle's, X, U, s within 1e-4, within 1e-6 where both sides end NLP OPTIMAL.  The
raised-Sw case is held to the rules of tests/test_gpu_inertia_shift.py.
"""
import numpy as np
import pytest

import oracle
import shift_cases as sc
import test_gpu_gram_valu as gv
import test_gpu_inertia_shift as gis

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402

N, C, KO, KN = 10, 2, 3, 8
INSTANCE = "12_4_1_10_2_11"

_cache = {}


def copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if v is not None}


def gpu_solve(b, use_nlp=1, solves=1, options=None, want_option=None, qp_init=None, form="", polish="", rows=slice(None),
              params=None, **kw):
    """Batch b (rows: a shard of it) at one wave an agent; the kernels' names are asserted before the outputs return."""
    A = b["x0"][rows].shape[0]
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=KO, K_nbr=KN, use_nlp=use_nlp, **(params or {})), A)
    try:
        s.set_waves(1)
        if qp_init is not None:
            s.set_qp_init(qp_init)
        for k, v in (options or {}).items():
            s.set_option(k, v)
        outs = []
        for _ in range(solves):
            out = s.solve(b["x0"][rows], b["ref"][rows], b["foot"][rows], b["obstacles"], b["nbr_state"],
                          qp_only=not use_nlp, **kw)
            assert s.last_kernels() == ("srb_nmpc_kernel_" + form + INSTANCE, polish), s.last_kernels()
            outs.append(copy(out))
        assert s.waves() == 1
        for k, v in (want_option or {}).items():
            assert s.get_option(k) == v, (k, s.get_option(k))
    finally:
        s.close()
    return outs if solves > 1 else outs[0]


def reference(key, b, **kw):
    """An oracle solve not among tests/test_gpu_gram_valu.py's, once per session (read only)."""
    if key not in _cache:
        r = oracle.solve_batch(oracle.params(N, C, K_obs=KO, K_nbr=KN, **kw), b["x0"], b["ref"], b["foot"], b["obstacles"],
                               b["nbr_state"], nthreads=8)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


@pytest.mark.parametrize("name", ["default", "crowded"])
def test_corrector_rhs_matches_oracle(name):
    """default: 64 agents; crowded: 16 agents at four times the obstacle density -- large z / s coefficients on the
    obstacle rows, and exits between a right-hand side and its use."""
    gv.check_parity(N, gpu_solve(gv.batch(name)), gv.reference(name))


@pytest.mark.parametrize("name", ["default", "crowded"])
def test_qp_copy_alone(name):
    """use_nlp = 0: the QP copy's corrector alone, nko = 0, the VAR and the mixed trip (under SRB_RHS_SLOTS_QP 1 their
    VEL and OBS slots carry a zero coefficient on a finite row; as shipped the copy keeps rhs_only beside the changed
    set_rhs lambda)."""
    r = gv.reference(name, use_nlp=0)
    gv.check_parity(N, gpu_solve(gv.batch(name), use_nlp=0), r, nlp=False)


def test_iswift_start():
    """qp_init = 0: iSWIFT's shifted start, duals of ~1e3 in the QP stage's first coefficients."""
    b = gv.batch("default")
    gv.check_parity(N, gpu_solve(b, qp_init=0), reference("qp_init0", b, qp_init=0))


def test_polish_kernel_stationarity():
    """polish_fused = 0, polish_waves = 1: srb_polish_kernel_12_4_1_10_2_11 runs polish_stationary through rhs_slots."""
    out = gpu_solve(gv.batch("default"), options={"polish_fused": 0, "polish_waves": 1}, want_option={"last_polish": 1.0},
                    polish="srb_polish_kernel_" + INSTANCE)
    gv.check_parity(N, out, gv.reference("default"))


def test_fp32_factor_form():
    """kkt_fp32_mu = 0.1: srb_nmpc_kernel_f32_12_4_1_10_2_11."""
    out = gpu_solve(gv.batch("default"), options={"kkt_fp32_mu": 0.1}, want_option={"last_kkt_fp32": 1.0}, form="f32_")
    gv.check_parity(N, out, gv.reference("default"))


def test_moving_obstacle_form():
    """srb_nmpc_kernel_mv_12_4_1_10_2_11 with a zero-velocity table computes what the plain instance does."""
    b = gv.batch("default")
    out = gpu_solve(b, form="mv_", obs_vel=np.zeros((b["obstacles"].shape[0], 2)))
    gv.check_parity(N, out, gv.reference("default"))


def shifted():
    """tests/shift_cases.py `default` (crowded, Sw raised) on a fresh context, once per session (read only)."""
    if "shifted" not in _cache:
        assert sc.LIP["default"][:6] == (N, C, KO, KN, 64, 1)
        _cache["shifted"] = gpu_solve(sc.lip_batch("default"), params=dict(Sw=sc.LIP["default"][8]))
    return _cache["shifted"]


def test_shifted_corrector_solve():
    """Raised Sw: the corrector's solve runs with delta != 0 behind the new g.  The rules of
    tests/test_gpu_inertia_shift.py test_shifted_batch_matches_oracle for its `default` case."""
    c = sc.lip_case("default")
    out, r = shifted(), c["r"]
    cmp = c["strict"] & c["shifted"]
    assert cmp.any()
    out0 = gpu_solve(sc.lip_batch("default"), params=dict(Sw=sc.SW_DEFAULT))
    assert (out["iters"][cmp, 1] != out0["iters"][cmp, 1]).any()
    gis.check_strict(N, out, r, cmp, "shifted strict agents")
    gis.check_strict(N, out, r, c["strict"], "strict agents")
    gis.check_every_agent("default", out, r, c["loose"])


def test_two_solves_on_one_context_are_bit_equal():
    o1, o2 = gpu_solve(gv.batch("default"), solves=2)
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k


def test_shards_are_bit_equal_to_the_full_batch():
    """Two unequal shards (agent_offset) of the raised-Sw batch against the whole neighbour table."""
    b, full = sc.lip_batch("default"), shifted()
    for lo, hi in ((0, 29), (29, 64)):
        part = gpu_solve(b, rows=slice(lo, hi), params=dict(Sw=sc.LIP["default"][8]), agent_offset=lo)
        for k in ("x", "x_qp", "obj", "status", "iters", "sel"):
            assert np.array_equal(part[k], full[k][lo:hi], equal_nan=True), (k, lo)


def test_nan_neighbour_row_stays_out_of_g():
    """One NaN row appended to the neighbour table: never selected, so no masked row may reach g as a NaN through the
    coefficient path -- finite outputs and the oracle's statuses."""
    b = dict(gv.batch("crowded"))
    b["nbr_state"] = np.vstack([b["nbr_state"], np.full((1, 4), np.nan)])
    r = reference("nan_row", b)
    out = gpu_solve(b)
    for k in ("x", "x_qp", "obj"):
        assert np.isfinite(out[k]).all(), k
    print("max |x - oracle|:", np.abs(gv.xus(N, out["x"]) - gv.xus(N, r["x"])).max(), "counts equal",
          bool((out["iters"] == r["iters"]).all()))
    np.testing.assert_array_equal(out["status"], r["status"])
