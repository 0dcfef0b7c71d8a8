"""GPU tests of the NLP stage's inertia shift in the SRB-12 solve kernel (csrc/srb12_kernels.hip: factor(delta),
refine(delta), Sw + delta in the slack's Schur complement), on the cases tests/shift_cases.py selects from the oracle
alone (crowded batches, the slack weight Sw raised until the condensed Hessian turns indefinite).

Rules.  Strict agents (stable under a 1e-12 perturbation of the oracle's inputs): status and iteration counts equal to
the oracle's in both columns, states and slack within 1e-6, forces within 1e-4 N -- the GPU parity rule of
tests/test_srb12.py.  Every agent: a documented status, finite outputs, and tests/test_srb12.py's KKT certificate at
its thresholds wherever the kernel reports NLP OPTIMAL; only loose agents may differ from the oracle in status.
"""
import numpy as np
import pytest

import oracle
import shift_cases as sc
from kkt import certify
from test_srb12 import _obs_for, _problem

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from srbnmpc import srb12  # noqa: E402

X_TOL, U_TOL = 1e-6, 1e-4                 # tests/test_srb12.py test_srb12_gpu_vs_oracle
DOCUMENTED = (0, 1, 2, 3, 4)
KEYS = ("x", "x_qp", "obj", "status", "iters", "sel")

_cache = {}


def gpu_params(name, **kw):
    N, Ko, Kn = sc.SRB12[name][:3]
    kw.setdefault("Sw", sc.SRB12[name][5])
    return sc.srb12_weights(srb12.default_params(N, K_obs=Ko, K_nbr=Kn), **kw)


def gpu_solve(name, solves=1, **kw):
    A, b = sc.SRB12[name][3], sc.srb12_batch(name)
    s = srb12.Solver12(gpu_params(name, **kw), A)
    try:
        outs = [{k: np.array(v, copy=True) for k, v in
                 s.solve(b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], b["nbr_state"]).items()}
                for _ in range(solves)]
    finally:
        s.close()
    return outs if solves > 1 else outs[0]


def solved(name):
    if name not in _cache:
        _cache[name] = gpu_solve(name)
    return _cache[name]


def check_strict(N, out, r, sel, what):
    ex = np.abs(out["x"][:, :12 * N] - r["x"][:, :12 * N]).max(1)
    eu = np.abs(out["x"][:, 12 * N:24 * N] - r["x"][:, 12 * N:24 * N]).max(1)
    es = np.abs(out["x"][:, -1] - r["x"][:, -1])
    bad = sel & ((out["status"] != r["status"]).any(1) | (out["iters"] != r["iters"]).any(1))
    print(f"{what}: compared {int(sel.sum())}, largest error states {ex[sel].max():.3e} forces {eu[sel].max():.3e} slack "
          f"{es[sel].max():.3e}, other status or count "
          f"{[(int(a), out['status'][a].tolist(), r['status'][a].tolist(), out['iters'][a].tolist(), r['iters'][a].tolist()) for a in np.nonzero(bad)[0]]}")
    assert not bad.any()
    assert ex[sel].max() < X_TOL and eu[sel].max() < U_TOL and es[sel].max() < X_TOL, (ex[sel].max(), eu[sel].max(), es[sel].max())


def check_every_agent(name, out, r, loose, **kw):
    b = sc.srb12_batch(name)
    p = sc.srb12_params(name, **kw)
    st = out["status"]
    assert np.isin(st, DOCUMENTED).all(), np.unique(st)
    for k in ("x", "x_qp", "obj"):
        assert np.isfinite(out[k]).all(), k                      # KKTFAIL / FATAL agents included
    worst = dict(stat_rel=0.0, prim=0.0, eq=0.0)
    for a in np.nonzero(st[:, 1] == 0)[0]:
        obs, eps = _obs_for(p, b, a)
        Pd, c, Aeq, beq, gJ, hh = _problem(p, b["x0"][a], b["xref"][a], b["foot"][a], b["contact"][a], obs, eps)
        cert = certify(Pd, c, Aeq, beq, gJ, hh, out["x"][a])
        worst = {k: max(worst[k], cert[k]) for k in worst}
        assert cert["eq"] < 1e-9 and cert["prim"] < 1e-7 and cert["stat_rel"] < 1e-6, (int(a), cert)
    differ = (st != r["status"]).any(1)
    print(f"{name}: NLP statuses {dict(zip(*[v.tolist() for v in np.unique(st[:, 1], return_counts=True)]))}, "
          f"{int((st[:, 1] == 0).sum())} certified OPTIMAL (worst {worst}), "
          f"{int(differ.sum())} of {int(loose.sum())} loose agents differ from the oracle in status")
    assert not (differ & ~loose).any(), np.nonzero(differ & ~loose)[0]


@pytest.mark.parametrize("name", list(sc.SRB12))
def test_srb12_shifted_batch_matches_oracle(name):
    c = sc.srb12_case(name)
    N = sc.SRB12[name][0]
    out, r = solved(name), c["r"]
    cmp = c["strict"] & c["shifted"]
    print(f"{name}: {int(c['shifted'].sum())} shifted agents, {int(cmp.sum())} of them strict, {int(c['strict'].sum())} "
          f"strict of {cmp.size}; oracle tries up to {int(r['stats']['max_tries'].max())}, delta up to "
          f"{r['stats']['max_delta'].max():.3g}")
    assert cmp.any()
    out0 = gpu_solve(name, Sw=sc.SW_DEFAULT)
    assert (out["iters"][cmp, 1] != out0["iters"][cmp, 1]).any()       # the override reached the kernel
    check_strict(N, out, r, cmp, name + " shifted strict agents")
    check_strict(N, out, r, c["strict"], name + " strict agents")
    check_every_agent(name, out, r, c["loose"])


def test_srb12_non_default_weights_without_a_shift():
    """q, qN, r and Sw all off their defaults, no agent shifted: every agent under the strict rule."""
    c = sc.srb12_weights_case()
    assert not c["r"]["stats"]["failed"].any() and c["strict"].all()
    out = gpu_solve("n10", **sc.SRB12_WEIGHTS)
    check_strict(10, out, c["r"], c["strict"], "non-default weights")
    check_every_agent("n10", out, c["r"], ~c["strict"], **sc.SRB12_WEIGHTS)
    # the overrides reached the kernel: not the solution of the same batch at the default weights
    assert np.abs(out["x"] - sc.srb12_case("n10")["r0"]["x"]).max() > 1e-3


def test_srb12_two_solves_of_a_shifted_batch_are_bit_equal():
    o1, o2 = gpu_solve("n10", solves=2)
    for k in KEYS:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
        assert np.array_equal(o1[k], solved("n10")[k], equal_nan=True), k


def test_srb12_shards_and_device_entry_on_a_shifted_batch():
    """Two shards (agent_offset) bit equal to the full batch, and solve_device bit equal to solve."""
    name = "n10"
    A, b, full = sc.SRB12[name][3], sc.srb12_batch(name), solved(name)
    prm = gpu_params(name)
    s = srb12.Solver12(prm, A)
    try:
        for lo, hi in ((0, 13), (13, A)):
            part = s.solve(b["x0"][lo:hi], b["xref"][lo:hi], b["foot"][lo:hi], b["contact"][lo:hi], b["obstacles"],
                           b["nbr_state"], agent_offset=lo)
            for k in KEYS:
                assert np.array_equal(part[k], full[k][lo:hi], equal_nan=True), (k, lo)
        T = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device="cuda")
        f8, i4 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        o = dict(x_qp=torch.zeros(A, prm.nv, **f8), x=torch.zeros(A, prm.nv, **f8), obj=torch.zeros(A, **f8),
                 status=torch.zeros(A, 2, **i4), iters=torch.zeros(A, 2, **i4))
        s.solve_device(T(b["x0"]), T(b["xref"]), T(b["foot"]), T(b["contact"], torch.int32), T(b["obstacles"]),
                       T(b["nbr_state"]), o)
        torch.cuda.synchronize()
        for k in o:
            assert np.array_equal(o[k].cpu().numpy(), full[k], equal_nan=True), k
    finally:
        s.close()
