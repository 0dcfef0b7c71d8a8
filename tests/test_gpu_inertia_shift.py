"""GPU tests of the NLP stage's inertia shift in the LIP solve kernel (csrc/srb_kernels.hip, the `ntries` loop: gj_load's
H0 + delta Z'Z, la_solve's shifted refinement residual, ZZ holding Z'Z by the time a shift reads it, the uniform failure
branch, the `near && delta != 0` exit), on the cases tests/shift_cases.py selects from the oracle alone: crowded batches
with the slack weight Sw raised until the reduced Newton matrix turns indefinite.

Rules.  Strict agents (stable under a 1e-12 perturbation of the oracle's inputs): status and iteration counts equal to
the oracle's in both columns, X, U, s within 1e-4, within 1e-6 where both sides end NLP OPTIMAL -- the rule of
tests/test_gpu_factor_chain.py.  Every agent: a documented status, finite outputs, and the solver-independent KKT
certificate (tests/kkt.py, thresholds of tests/test_gpu_parity.py) wherever the kernel reports NLP OPTIMAL; only loose
agents may differ from the oracle in status.  Every case proves from the oracle's statistics that shifted agents were
among the strict ones compared, and from a default-Sw solve that the override reached the kernel.
"""
import numpy as np
import pytest

import oracle
import shift_cases as sc
from kkt import certify, nlp_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402

NLP_TOL = 1e-4
POLISHED_TOL = 1e-6
CERT_STAT, CERT_PRIM = 1e-5, 1e-6        # tests/test_gpu_parity.py
DOCUMENTED = (0, 1, 2, 3, 4)

_cache = {}


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items() if v is not None}


def gpu_solve(name, fused=1, solves=1, **weights):
    """The case's batch on a fresh context (weights: Params overrides; default: the case's Sw)."""
    N, C, Ko, Kn, A, waves, want = sc.LIP[name][:7]
    weights.setdefault("Sw", sc.LIP[name][8])
    b = sc.lip_batch(name)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=1, **weights), A)
    try:
        s.set_waves(waves)
        s.set_option("polish_fused", fused)
        outs = [copy(s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])) for _ in range(solves)]
        assert s.waves() == want
    finally:
        s.close()
    return outs if solves > 1 else outs[0]


def solved(name):
    """The case's fused solve, once per session (read only)."""
    if name not in _cache:
        _cache[name] = gpu_solve(name)
    return _cache[name]


def check_strict(N, out, r, sel, what):
    """The strict rule on the agents `sel`; returns the largest error among them."""
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    bad = sel & ((out["status"] != r["status"]).any(1) | (out["iters"] != r["iters"]).any(1))
    print(f"{what}: compared {int(sel.sum())}, largest |x - oracle| {e[sel].max():.3e}, other status or count "
          f"{[(int(a), out['status'][a].tolist(), r['status'][a].tolist(), out['iters'][a].tolist(), r['iters'][a].tolist()) for a in np.nonzero(bad)[0]]}")
    assert not bad.any()
    assert e[sel].max() < NLP_TOL, (int(np.argmax(e * sel)), float(e[sel].max()))
    both = sel & (out["status"][:, 1] == 0) & (r["status"][:, 1] == 0)
    if both.any():
        assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))
    return float(e[sel].max())


def check_every_agent(name, out, r, loose, **weights):
    N, C, Ko, Kn = sc.LIP[name][:4]
    b = sc.lip_batch(name)
    weights.setdefault("Sw", sc.LIP[name][8])
    st = out["status"]
    assert np.isin(st, DOCUMENTED).all(), np.unique(st)
    for k in ("x", "x_qp", "obj"):
        assert np.isfinite(out[k]).all(), k                      # KKTFAIL / FATAL agents included
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn, **weights)
    worst = dict(stat_rel=0.0, prim=0.0)
    for a in np.nonzero(st[:, 1] == 0)[0]:
        obs, eps = oracle.select_obstacles(op, b["x0"][a], b["obstacles"], b["nbr_state"], int(a))
        Pd, c, Aeq, beq, G, h = oracle.build_qp(op, b["x0"][a], b["ref"][a], b["foot"][a])
        gJ, hh = nlp_rows(N, C, Pd.size, G, h, obs, eps, op.vsat)
        cert = certify(Pd, c, Aeq, beq, gJ, hh, out["x"][a])
        worst = {k: max(worst[k], cert[k]) for k in worst}
        assert cert["stat_rel"] < CERT_STAT and cert["prim"] < CERT_PRIM, (int(a), cert)
    differ = (st != r["status"]).any(1)
    print(f"{name}: NLP statuses {dict(zip(*[v.tolist() for v in np.unique(st[:, 1], return_counts=True)]))}, "
          f"{int((st[:, 1] == 0).sum())} certified OPTIMAL (worst {worst}), "
          f"{int(differ.sum())} of {int(loose.sum())} loose agents differ from the oracle in status")
    assert not (differ & ~loose).any(), np.nonzero(differ & ~loose)[0]


@pytest.mark.parametrize("name", list(sc.LIP))
def test_shifted_batch_matches_oracle(name):
    c = sc.lip_case(name)
    N = sc.LIP[name][0]
    out, r = solved(name), c["r"]
    cmp = c["strict"] & c["shifted"]
    print(f"{name}: {int(c['shifted'].sum())} shifted agents, {int(cmp.sum())} of them strict, {int(c['strict'].sum())} "
          f"strict of {cmp.size}; oracle tries up to {int(r['stats']['max_tries'].max())}, delta up to "
          f"{r['stats']['max_delta'].max():.3g}")
    # the path was exercised: shifted agents are among the compared ones, and the kernel's own iteration counts on
    # them are not those of the same batch at the default Sw
    assert cmp.any()
    out0 = gpu_solve(name, Sw=sc.SW_DEFAULT)
    assert (out["iters"][cmp, 1] != out0["iters"][cmp, 1]).any()
    check_strict(N, out, r, cmp, name + " shifted strict agents")
    check_strict(N, out, r, c["strict"], name + " strict agents")
    check_every_agent(name, out, r, c["loose"])
    if name in sc.LIP_EXITS:
        rule, status = sc.LIP_EXITS[name]
        hit = cmp & (r["stats"]["exit"] == oracle.EXIT_RULES.index(rule))
        assert hit.any() and (out["status"][hit, 1] == status).all()


def test_non_default_weights_without_a_shift():
    """Qw, Pw, Rw, Sw and eps_obs all off their defaults, no agent shifted: every agent under the strict rule."""
    c = sc.lip_weights_case()
    assert not c["r"]["stats"]["failed"].any() and c["strict"].all()
    out = gpu_solve("default", **sc.LIP_WEIGHTS)
    check_strict(10, out, c["r"], c["strict"], "non-default weights")
    check_every_agent("default", out, c["r"], ~c["strict"], **sc.LIP_WEIGHTS)
    # the overrides reached the kernel: not the solution of the same batch at the default weights
    assert np.abs(xus(10, out["x"]) - xus(10, sc.lip_case("default")["r0"]["x"])).max() > 1e-3


def test_two_solves_of_a_shifted_batch_are_bit_equal():
    o1, o2 = gpu_solve("default", solves=2)
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
    for k in o1:                                                  # and a fresh context gives the same bits
        assert np.array_equal(o1[k], solved("default")[k], equal_nan=True), k


def test_shards_of_a_shifted_batch_are_bit_equal_to_the_full_batch():
    """Two shards (agent_offset) against the whole neighbour table, one context."""
    N, C, Ko, Kn, A = sc.LIP["default"][:5]
    b, full = sc.lip_batch("default"), solved("default")
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, Sw=sc.LIP["default"][8]), A)
    try:
        s.set_waves(sc.LIP["default"][5])                         # the case's waves per agent, as the full solve
        for lo, hi in ((0, 29), (29, A)):                         # unequal shards, neither a multiple of the wave's agents
            part = s.solve(b["x0"][lo:hi], b["ref"][lo:hi], b["foot"][lo:hi], b["obstacles"], b["nbr_state"], agent_offset=lo)
            for k in ("x", "x_qp", "obj", "status", "iters", "sel"):
                assert np.array_equal(part[k], full[k][lo:hi], equal_nan=True), (k, lo)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["default", "n20"])
def test_polish_kernel_equals_fused_polish_on_a_shifted_batch(name):
    """polish_fused 0 (srb_polish_kernel) against 1: the same statuses and counts, and the polished points within the
    polished tolerance.  In n20 the oracle rejects a polish whose reduced matrix is not positive definite."""
    if name == "n20":
        assert sc.lip_case(name)["r"]["stats"]["polish_npd"].any()
    N = sc.LIP[name][0]
    f1, f0 = solved(name), gpu_solve(name, fused=0)
    e = np.abs(xus(N, f1["x"]) - xus(N, f0["x"])).max(1)
    print(f"{name}: fused against polish kernel, largest difference {e.max():.3e}, bit equal {np.array_equal(f1['x'], f0['x'])}")
    np.testing.assert_array_equal(f0["status"], f1["status"])
    np.testing.assert_array_equal(f0["iters"], f1["iters"])
    assert e.max() < POLISHED_TOL
    c = sc.lip_case(name)
    check_strict(N, f0, c["r"], c["strict"], name + " polish kernel, strict agents")


def test_device_entry_equals_host_entry_on_a_shifted_batch():
    N, C, Ko, Kn, A = sc.LIP["default"][:5]
    b, h = sc.lip_batch("default"), solved("default")
    prm = srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn, Sw=sc.LIP["default"][8])
    s = srbnmpc.BatchSolver(prm, A)
    try:
        s.set_waves(sc.LIP["default"][5])
        T = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
        f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        o = dict(x_qp=torch.zeros(A, prm.nv, **f8), x=torch.zeros(A, prm.nv, **f8), obj=torch.zeros(A, **f8),
                 status=torch.zeros(A, 2, **i4), iters=torch.zeros(A, 2, **i4))
        s.solve_device(T(b["x0"]), T(b["ref"].reshape(A, -1)), T(b["foot"].reshape(A, -1)), T(b["obstacles"]),
                       T(b["nbr_state"]), o)
        torch.cuda.synchronize()
        for k in o:
            assert np.array_equal(o[k].cpu().numpy(), h[k], equal_nan=True), k
    finally:
        s.close()
