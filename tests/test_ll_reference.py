"""CPU tests of the extended-precision reference of the low-level CLF-QP (tests/ll_reference.py) and of
the stress cases (tests/ll_cases.py).

  * reference against the fp64 oracle, iterate by iterate: a gate on both staying the same algorithm
    (1e-5 relative; the oracle's measured drift on the stiff cases is up to 4e-7), and agreement on
    (status, iters) in at least 75 % of the agents of every case.  The reference never ends at MAXIT:
    the oracle's MAXIT exits on these cases are rounding artefacts of its reduced fp64 solve;
  * coverage: the cases do make torque bounds, cone rows and the CLF row active (counts below), and the
    default workload makes no torque bound active -- the gap the cases close;
  * the reference reproduces the genuine-iSWIFT goldens (flag, iterations, x to 1e-8).
"""
import os

import numpy as np
import pytest

import oracle

import ll_cases
import ll_reference

if not ll_reference.EXTENDED:
    pytest.skip(ll_reference.NOT_EXTENDED, allow_module_level=True)

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ll_ctrl.npz")
TRAJ_GATE = 1e-5
X_TOL = 1e-8

# minimum number of agents (of 24) with an active row of the family at the reference's final point
MIN_ACTIVE = {
    "track5": dict(torque=5),
    "track5_noclf": dict(torque=5),
    "dh50": dict(torque=12, clf=5),
    "mu01": dict(friction=12),
    "mu0": dict(friction=12),
    "gains": dict(clf=8),
}


@pytest.mark.parametrize("case", list(ll_cases.CASES))
def test_ll_reference_matches_oracle_per_iteration(case):
    t = ll_cases.trajectories(case)
    A = ll_cases.A
    assert (t["ref_flag"] == ll_reference.OPTIMAL).all(), t["ref_flag"]
    agree = (t["ref_flag"] == t["orc_flag"]) & (t["ref_it"] == t["orc_it"])
    print(f"{case}: disagree {A - agree.sum()}  E_orc {t['E_orc']:.2e}  active "
          + " ".join(f"{k} {v.sum()}" for k, v in t["active"].items()))
    assert agree.sum() >= 0.75 * A, (t["ref_flag"], t["orc_flag"], t["ref_it"], t["orc_it"])
    for a in range(A):
        for k in range(min(t["ref_it"][a], t["orc_it"][a]) + 1):
            e = ll_cases.rel_err(t["orc_x"][k, a], t["ref_x"][a][k])
            assert e <= TRAJ_GATE, (a, k, e)


@pytest.mark.parametrize("case", list(ll_cases.CASES))
def test_ll_cases_reach_the_bounds(case):
    act = ll_cases.trajectories(case)["active"]
    for fam, least in MIN_ACTIVE.get(case, {}).items():
        assert act[fam].sum() >= least, (case, fam, act[fam].sum())
    if case == "default":
        # the workload of the older tests: no torque bound is ever active on it
        assert act["torque"].sum() == 0


@pytest.mark.parametrize("clf", [1, 0])
def test_ll_reference_matches_genuine_iswift(clf):
    gz = np.load(GOLD, allow_pickle=False)
    g = {k: gz[k] for k in gz.files}
    p = oracle.ll_params(useCLF=clf)
    for a in range(g["ind"].shape[0]):
        Pd, c, A, b, G, h, *_ = oracle.ll_build_qp(p, g, a)
        xs, f, it = ll_reference.ipm_ld(Pd, c, A, b, G, h, p.maxit, p.tol)
        assert f == g[f"iswift_flag_clf{clf}"][a] and it == g[f"iswift_iters_clf{clf}"][a]
        assert np.abs(xs[-1] - g[f"iswift_x_clf{clf}"][a][:xs[-1].size]).max() < X_TOL
