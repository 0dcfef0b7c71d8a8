"""GPU tests of the low-level CLF-QP kernel (srb_ll_kernel) where its hand-made linear algebra is hard:
active torque bounds, cone rows and CLF row, every parameter off its default, non-zero tau
(tests/ll_cases.py), judged iterate by iterate against the extended-precision reference
(tests/ll_reference.py).

Tolerances (written here):
  * trajectory: for every agent and k <= min(it_ref, it_oracle, it_gpu),
        max|x_gpu(k) - x_ref(k)| / max(1, ||x_ref(k)||_inf) <= B(case) = max(1e-8, 10 E_orc(case)),
    E_orc the fp64 oracle's worst such distance from the reference on the case (computed here from the
    oracle and the reference, never from the GPU); 1e-8 is the project's X_TOL; the factor 10 because two
    fp64 factorisations of one ill-conditioned system err by cond * eps with different constants;
  * exit: (status, iters) is the reference's or the oracle's (the oracle's MAXIT stalls on these cases are
    rounding artefacts, which the kernel's solve may or may not share); never FAILED or FATAL; where the
    kernel and the reference are both OPTIMAL, max|x_gpu - x_ref| <= Bf(case) = max(1e-8, 10 E_fin(case)) in
    absolute terms, E_fin the oracle's own worst max|x_orc - x_ref| at the final point over the agents where
    oracle and reference are OPTIMAL after the same number of iterations (computed here, never from the GPU; the
    same construction as B(case)).  The plain 1e-8 is out of fp64's reach where x is large: on track5_noclf
    (|x|_inf = 2.7e2) the oracle is 1.2e-8 from the reference and the kernel 2.3e-8, against Bf = 1.2e-7; on
    track5 6.1e-9 and 7.4e-9, on mu0 1.6e-9 and 5.8e-9; on the seven other cases both are below 1e-9 and
    Bf = 1e-8 (profiles/ll_stress_errors.txt);
  * epilogue from the kernel's own x (tau, QP_force, ddq, dq, q): rtol 1e-10, atol 1e-9, the tolerances
    tests/test_ll_oracle.py uses for the same formulas; V to 1e-10 max(1, |V|); dV = LfV + Veps + LgV'aux
    to 1e-9 max(1, |LfV| + |Veps| + sum|LgV_i aux_i|) (an fp64 sum of at most 20 such terms errs by
    20 * 2^-53 of that magnitude; 1e-9 is the bound test_ll_oracle.py puts on LfV alone).
The run with maxit = k must be the prefix of the full run: iters = min(k, iters_full), MAXIT exactly while
k <= iters_full (the exit test stands at the head of the next iteration, in iSWIFT, the oracle and the kernel
alike) or where the full run ends at MAXIT itself, and bit-identical outputs from k = iters_full on.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import lowlevel  # noqa: E402

import ll_cases  # noqa: E402
import ll_reference  # noqa: E402

if not ll_reference.EXTENDED:
    pytest.skip(ll_reference.NOT_EXTENDED, allow_module_level=True)

X_TOL = 1e-8
A = ll_cases.A
CASES = list(ll_cases.CASES)


def _bound(t):
    return max(X_TOL, 10.0 * t["E_orc"])


@pytest.mark.parametrize("case", CASES)
def test_ll_gpu_stress_trajectory(case):
    t = ll_cases.trajectories(case)
    B = _bound(t)
    errs = ll_cases.gpu_errors(case)["errs"]          # by agent, by iteration
    worst, a_w = max((float(e.max()), a) for a, e in enumerate(errs))
    print(f"{case}: E_orc {t['E_orc']:.2e}  bound {B:.2e}  gpu worst {worst:.2e} (agent {a_w}, k {int(errs[a_w].argmax())})")
    # first iteration over the bound, per agent: localises a fault
    first = {a: int(np.argmax(e > B)) for a, e in enumerate(errs) if (e > B).any()}
    assert not first, (f"bound {B:.2e}, worst {worst:.2e}; agent -> first iteration over the bound", first)


@pytest.mark.parametrize("case", CASES)
def test_ll_gpu_stress_prefix_property(case):
    runs = ll_cases.gpu_runs(case)
    full = runs[-1]
    for k, r in enumerate(runs):
        assert (r["iters"] == np.minimum(k, full["iters"])).all(), (k, r["iters"], full["iters"])
        # the exit test stands at the head of an iteration (Prime.c:150-160, as in the oracle): the run that
        # converges after iters_full steps sees it only when a further iteration is allowed, so maxit =
        # iters_full still ends at MAXIT, at the converged point
        maxit = (k <= full["iters"]) | (full["status"] == 2)
        assert ((r["status"] == 2) == maxit).all(), (k, r["status"], full["status"])
        assert (r["status"][~maxit] == full["status"][~maxit]).all()
        done = k >= full["iters"]
        for key in ("x", "tau", "QP_force", "ddq", "dq", "q", "V", "dV"):
            np.testing.assert_array_equal(r[key][done], full[key][done], err_msg=f"{key} at maxit {k}")
    orc = ll_cases.trajectories(case)
    o_it = orc["orc_it"]
    assert (orc["orc_x"][o_it, np.arange(A)] == orc["orc_x"][-1]).all()     # the oracle's runs are prefixes too


@pytest.mark.parametrize("case", CASES)
def test_ll_gpu_stress_exit(case):
    t, full = ll_cases.trajectories(case), ll_cases.gpu_runs(case)[-1]
    e = ll_cases.gpu_errors(case)
    Bf = ll_cases.final_bound(case)
    print(f"{case}: final |x - x_ref| kernel {e['e_final']:.2e} oracle {e['orc_final']:.2e} bound {Bf:.2e}; exits as "
          f"reference {e['as_ref'].sum()} as oracle {e['as_orc'].sum()} neither {e['neither']}")
    assert not np.isin(full["status"], (1, 3)).any(), full["status"]
    assert (e["as_ref"] | e["as_orc"]).all(), (full["status"], full["iters"], t["ref_flag"], t["ref_it"], t["orc_flag"],
                                               t["orc_it"])
    over = {a: float(e["final_abs"][a]) for a in range(A) if e["both"][a] and not e["final_abs"][a] <= Bf}
    assert not over, (f"bound {Bf:.2e} (oracle {e['orc_final']:.2e}); agent -> max|x - x_ref|", over)


@pytest.mark.parametrize("case", CASES)
def test_ll_gpu_stress_epilogue_from_own_x(case):
    runs = ll_cases.gpu_runs(case)
    prm, batch = ll_cases.case_params(case), ll_cases.case_batch(case)
    p = lowlevel.default_params(**prm)
    stand = 0
    for r in (runs[-1], runs[2]):      # the final point and an early iterate far from it
        for a in range(A):
            x = r["x"][a]
            e = ll_reference.epilogue_np(batch, a, x)
            np.testing.assert_array_equal(r["QP_force"][a], e["QP_force"])
            for key in ("tau", "ddq", "dq", "q"):
                np.testing.assert_allclose(r[key][a], e[key], rtol=1e-10, atol=1e-9, err_msg=f"{key} agent {a}")
            ind = batch["ind"][a]
            if (ind == 1).all():       # no swing leg: tau[0:6] is the caller's, untouched
                np.testing.assert_array_equal(r["tau"][a, :6], batch["tau"][a, :6])
                assert np.abs(batch["tau"][a, :6]).min() > 0
                stand += 1
            if not p.useCLF:
                assert r["V"][a] == 0 and r["dV"][a] == 0
                continue
            out = 6 + 3 * int((ind == 0).sum())
            con = 3 * int((ind == 1).sum())
            V, LfV, Veps, LgV = ll_reference.clf_np(p.kp, p.kd, p.clfEps, batch["y"][a][:out], batch["dy"][a][:out])
            aux = x[con + 12:con + 12 + out]
            assert abs(r["V"][a] - V) <= 1e-10 * max(1.0, abs(V)), (a, r["V"][a], V)
            mag = abs(LfV) + abs(Veps) + np.abs(LgV * aux).sum()
            assert abs(r["dV"][a] - (LfV + Veps + LgV @ aux)) <= 1e-9 * max(1.0, mag), (a, r["dV"][a], LfV + Veps + LgV @ aux)
    assert stand >= 2


def _device_call(c, b, with_x):
    dev = {"ind": torch.from_numpy(np.ascontiguousarray(b["ind"], np.int32)).cuda()}
    for k in lowlevel.IN_KEYS:
        dev[k] = torch.from_numpy(np.ascontiguousarray(b[k], np.float64).reshape(A, -1)).cuda()
    out = {k: torch.zeros((A, s), dtype=torch.float64, device="cuda") for k, s in lowlevel.OUT_SIZE.items()
           if with_x or k != "x"}
    out["tau"].copy_(torch.from_numpy(np.ascontiguousarray(b["tau"], np.float64)))
    out["status"] = torch.full((A,), -1, dtype=torch.int32, device="cuda")
    out["iters"] = torch.full((A,), -1, dtype=torch.int32, device="cuda")
    c.calc_torque_device(dev, out)
    c.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_ll_gpu_device_call_without_x_buffer():
    """x is the C ABI's optional output: without it every other output is bit-equal to a call with it."""
    b = ll_cases.case_batch("dh50")
    c = srbnmpc.LowLevelCtrl(lowlevel.default_params(), max_agents=A)
    try:
        w = _device_call(c, b, True)
        wo = _device_call(c, b, False)
    finally:
        c.close()
    assert "x" not in wo and np.abs(w["x"]).max() > 0
    assert (w["status"] != -1).all()
    for k in wo:
        np.testing.assert_array_equal(wo[k], w[k], err_msg=k)
    host = ll_cases.gpu_runs("dh50")[-1]
    for k in wo:
        np.testing.assert_array_equal(wo[k].reshape(host[k].shape), host[k], err_msg=k)


_BAD = [(f, v) for f in ("kp", "kd", "clfEps", "tauPen", "dfPen", "auxPen", "clfPen", "tol")
        for v in (0.0, -1.0, float("nan"))] + [("mu", -0.1), ("mu", float("nan")), ("maxit", -1)]


@pytest.mark.parametrize("field,value", _BAD, ids=[f"{f}={v}" for f, v in _BAD])
def test_ll_gpu_ctx_create_rejects_out_of_range(field, value):
    with pytest.raises(RuntimeError):
        srbnmpc.LowLevelCtrl(lowlevel.default_params(**{field: value}), max_agents=4).close()


def test_ll_gpu_zero_clf_penalty_is_accepted_without_the_clf():
    b = ll_cases.case_batch("track5_noclf")
    c = srbnmpc.LowLevelCtrl(lowlevel.default_params(useCLF=0, clfPen=0.0), max_agents=A)
    try:
        out = c.calc_torque(b)
    finally:
        c.close()
    ref = ll_cases.gpu_runs("track5_noclf")[-1]      # the same solve with the default clfPen, unused without the CLF
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.isfinite(out["x"]).all() and not np.isin(out["status"], (1, 3)).any()
