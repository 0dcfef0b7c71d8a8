"""Stress cases of the low-level CLF-QP: inputs and parameters that put every family of inequality rows
(friction cone, torque bounds, CLF) at its bound and move every parameter off its default.

ll_workload.make_batch builds inputs whose IO linearisation is achievable inside the torque limits: on
them no torque bound is ever active.  The cases here scale the tracking errors, shift dH0 or tighten the
cone until the bounds bind (tests/test_ll_reference.py asserts the counts).

  CASES            name -> (parameter overrides, input transform)
  case_batch       the inputs of a case (24 agents, tau non-zero so that its pass-through is visible)
  trajectories     per case, computed once per process: the extended-precision reference's iterates
                   (ll_reference.ipm_ld), the fp64 oracle's iterates (one run per maxit = k), E_orc and
                   the rows active at the reference's final point
"""
import numpy as np

import oracle
from srbnmpc import ll_workload

import ll_reference

A = 24
ACTIVE_SLACK = 1e-6


def _track5(b):
    b["y"] = b["y"] * 5
    b["dy"] = b["dy"] * 5


def _dh50(b):
    d = b["dH0"]
    b["dH0"] = d + 50 * np.random.default_rng(1).standard_normal(d.shape) * (d != 0)


def _base(b):
    pass


CASES = {
    "default": ({}, _base),
    "track5": ({}, _track5),
    "track5_noclf": (dict(useCLF=0), _track5),
    "dh50": ({}, _dh50),
    "mu01": (dict(mu=0.1), _base),
    "mu0": (dict(mu=0.0), _base),
    "gains": (dict(kp=100.0, kd=10.0, clfEps=0.3), _base),
    "penalties": (dict(tauPen=1e-2, dfPen=1.0, auxPen=1e4, clfPen=1e5), _base),
    "tol8": (dict(tol=1e-8, maxit=40), _base),
    "mixed": (dict(mu=0.2, kp=300.0, kd=25.0, clfEps=0.5), _track5),
}


def base_batch():
    ind = np.random.default_rng(0).integers(0, 2, (A, 4)).astype(np.int32)
    ind[:6] = [[0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0], [0, 1, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0]]
    b = ll_workload.make_batch(A, seed=200, ind=ind)
    b["tau"] = np.random.default_rng(3).uniform(-5, 5, (A, 18))
    return b


def case_params(name):
    return dict(CASES[name][0])


def case_batch(name):
    b = base_batch()
    CASES[name][1](b)
    return b


def case_maxit(name):
    return int(case_params(name).get("maxit", oracle.ll_params().maxit))


def rel_err(x, xref):
    """max|x - xref| / max(1, ||xref||_inf) along the last axis"""
    return np.abs(x - xref).max(-1) / np.maximum(1.0, np.abs(xref).max(-1))


_traj = {}
_gpu = {}


def gpu_runs(name):
    """The kernel's run of the case with maxit = k for k = 0..maxit (one small context each, closed after its
    launch), computed once per process: list of calc_torque output dicts, index k."""
    if name not in _gpu:
        import srbnmpc
        from srbnmpc import lowlevel
        prm, batch = case_params(name), case_batch(name)
        runs = []
        for k in range(case_maxit(name) + 1):
            c = srbnmpc.LowLevelCtrl(lowlevel.default_params(**dict(prm, maxit=k)), max_agents=A)
            try:
                runs.append(c.calc_torque(batch))
            finally:
                c.close()
        _gpu[name] = runs
    return _gpu[name]


def iterate_errors(name, x_of_k, iters):
    """rel_err of x_of_k(k)[a] from the reference's iterate k, for every agent a and k <= min(it_ref, it_orc,
    iters[a]): list (by agent) of arrays (by k)"""
    t = trajectories(name)
    return [np.array([float(rel_err(x_of_k(k)[a], t["ref_x"][a][k]))
                      for k in range(min(t["ref_it"][a], t["orc_it"][a], iters[a]) + 1)]) for a in range(A)]


def final_bound(name):
    """Absolute bound on max|x - x_ref| at the final point: max(1e-8, 10 x the oracle's own worst absolute distance
    from the reference there), over the agents where oracle and reference are OPTIMAL after the same number of
    iterations -- B(case) of the trajectory, in the absolute measure of the project's X_TOL."""
    return max(1e-8, 10.0 * trajectories(name)["E_orc_final"])


def gpu_errors(name):
    """The figures of profiles/ll_stress_errors.txt for one case: E_orc, the kernel's iterate errors (errs, by agent
    and k; e_traj their worst), its final-point errors where it and the reference are both OPTIMAL (final_abs by
    agent, e_final their worst, e_final_rel scaled), the oracle's (orc_final), and how the exits split between the
    reference and the oracle."""
    t, runs = trajectories(name), gpu_runs(name)
    full = runs[-1]
    errs = iterate_errors(name, lambda k: runs[k]["x"], full["iters"])
    both = (full["status"] == 0) & (t["ref_flag"] == 0)
    fin = np.array([np.abs(full["x"][a] - t["ref_x"][a][-1]).max() for a in range(A)])
    fin_rel = np.array([float(rel_err(full["x"][a], t["ref_x"][a][-1])) for a in range(A)])
    as_ref = (full["status"] == t["ref_flag"]) & (full["iters"] == t["ref_it"])
    as_orc = (full["status"] == t["orc_flag"]) & (full["iters"] == t["orc_it"])
    split = (t["ref_flag"] != t["orc_flag"]) | (t["ref_it"] != t["orc_it"])
    return dict(E_orc=t["E_orc"], errs=errs, e_traj=max(float(e.max()) for e in errs), final_abs=fin, both=both,
                e_final=float(fin[both].max()) if both.any() else 0.0,
                e_final_rel=float(fin_rel[both].max()) if both.any() else 0.0, orc_final=t["E_orc_final"],
                as_ref=as_ref, as_orc=as_orc, split=int(split.sum()), with_ref=int((split & as_ref).sum()),
                with_orc=int((split & as_orc).sum()), neither=int((~as_ref & ~as_orc).sum()),
                orc_stall=int((t["orc_flag"] == 2).sum()))


def trajectories(name):
    """dict of
      batch, params, maxit
      ref_x [A][k] (32, zero padded), ref_flag [A], ref_it [A]      extended-precision reference
      orc_x [maxit + 1, A, 32]  oracle's x of the run with maxit = k;  orc_flag, orc_it [A] of the full run
      E_orc    the oracle's worst rel_err from the reference over all agents and k <= min(it_ref, it_orc)
      E_orc_final  the oracle's worst max|x - x_ref| at the final point, over the agents where both are OPTIMAL
               after the same number of iterations
      active   dict friction / torque / clf -> bool [A]: a row of that family has slack < ACTIVE_SLACK at the
               reference's final point
    """
    if name in _traj:
        return _traj[name]
    prm, batch, maxit = case_params(name), case_batch(name), case_maxit(name)
    p = oracle.ll_params(**prm)
    ref_x, ref_flag, ref_it = [], np.zeros(A, np.int32), np.zeros(A, np.int32)
    act = {k: np.zeros(A, bool) for k in ("friction", "torque", "clf")}
    for a in range(A):
        Pd, c, Am, bm, G, h, *_ = oracle.ll_build_qp(p, batch, a)
        xs, f, it = ll_reference.ipm_ld(Pd, c, Am, bm, G, h, maxit, p.tol)
        ref_x.append([np.pad(x, (0, 32 - x.size)) for x in xs])
        ref_flag[a], ref_it[a] = f, it
        slack = h - G @ xs[-1]
        nf = 5 * int((batch["ind"][a] == 1).sum())
        act["friction"][a] = (slack[:nf] < ACTIVE_SLACK).any()
        act["torque"][a] = (slack[nf:nf + 24] < ACTIVE_SLACK).any()
        act["clf"][a] = bool(p.useCLF) and slack[-1] < ACTIVE_SLACK
    orc_x = np.zeros((maxit + 1, A, 32))
    for k in range(maxit + 1):
        o = oracle.ll_calc_torque(oracle.ll_params(**dict(prm, maxit=k)), batch)
        orc_x[k] = o["x"]
    E, Ef = 0.0, 0.0
    for a in range(A):
        for k in range(min(ref_it[a], o["iters"][a]) + 1):
            E = max(E, float(rel_err(orc_x[k, a], ref_x[a][k])))
        if o["status"][a] == 0 and ref_flag[a] == 0 and o["iters"][a] == ref_it[a]:
            Ef = max(Ef, float(np.abs(orc_x[-1, a] - ref_x[a][-1]).max()))
    _traj[name] = dict(batch=batch, params=prm, maxit=maxit, ref_x=ref_x, ref_flag=ref_flag, ref_it=ref_it,
                       orc_x=orc_x, orc_flag=o["status"].copy(), orc_it=o["iters"].copy(), E_orc=E, E_orc_final=Ef,
                       active=act)
    return _traj[name]
