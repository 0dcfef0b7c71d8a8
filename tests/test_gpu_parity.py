"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the goldens.

Tolerances (written here, from SURVEY.md §8c / BASELINE.json north star):
  * QP stage: X, U, s within 1e-6 abs of the genuine iSWIFT (its own tolerance); in
    practice ~1e-8 and identical iteration counts.  lambda compared only for C = 2
    (non-unique for 4 contacts).
  * NLP stage: X, U, s within 1e-4 abs of the oracle / KKT-certified goldens (north star
    "||.||_inf < 1e-4"); in practice ~1e-8 with identical iteration counts.
"""
import numpy as np
import pytest
from conftest import converged, load_golden, ok_elem

import bench
import oracle
from kkt import certify, nlp_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402

QP_TOL = 1e-6
NLP_TOL = 1e-4


def conv(st):
    """Exit codes as compared between GPU and oracle: exactly (round 3: the active-set polish ends
    both at the exact KKT point as OPTIMAL, so ACCEPTABLE is no longer merged into OPTIMAL)."""
    return np.array(st, copy=True)


_solvers = {}


def solver(N, C, K_obs=1, K_nbr=0, use_nlp=1, max_agents=2048, qp_init=1, qp_warm_tol=None):
    key = (N, C, K_obs, K_nbr, use_nlp, max_agents, qp_init, qp_warm_tol)
    if key not in _solvers:
        p = srbnmpc.default_params(N, C, K_obs=K_obs, K_nbr=K_nbr, use_nlp=use_nlp)
        _solvers[key] = srbnmpc.BatchSolver(p, max_agents)
        _solvers[key].set_qp_init(qp_init)
        if qp_warm_tol is not None:
            _solvers[key].set_option("qp_warm_tol", qp_warm_tol)
    return _solvers[key]


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


# ----------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("qp_init", [0, 1])
def test_kat2_reference_instance(kat2, qp_init):
    """The reference's logged instance: QP stage == the reference's own logged output and
    genuine iSWIFT; NLP stage == KKT-certified optimum.  qp_init 0 (iSWIFT's start) follows the
    genuine iSWIFT step for step (same iteration count); the default scaled start ends at the same
    point to the log's precision in fewer iterations."""
    s = solver(4, 4, K_obs=1, qp_init=qp_init, qp_warm_tol=0.0)      # the QP stage to iSWIFT's tolerance
    foot = np.repeat(kat2["F"][None], 4, 0)
    out = s.solve(kat2["x0"][None], kat2["ref"][None], foot[None], np.asarray(kat2["obstacle"])[None])
    assert out["status"][0].tolist() == [0, 0]
    if qp_init == 0:
        assert out["iters"][0, 0] == kat2["iters_qp_qd"]
    else:
        assert out["iters"][0, 0] < kat2["iters_qp_qd"]
    xq = out["x_qp"][0]
    np.testing.assert_allclose(xq[:24], kat2["logged_qp_x"], atol=2e-9, rtol=0)
    np.testing.assert_allclose(xus(4, xq), xus(4, kat2["x_qp_iswift_qd"]), atol=1e-8, rtol=0)
    np.testing.assert_allclose(xus(4, out["x"][0]), xus(4, kat2["x_nlp"]), atol=1e-9, rtol=0)
    assert abs(out["obj"][0] - kat2["obj_nlp"]) < 1e-8


@pytest.mark.parametrize("qp_init", [0, 1])
def test_qp_random_vs_genuine_iswift(qp_init):
    """QP stage (use_snopt == false) against the genuine iSWIFT.  qp_init 0: iSWIFT's own start,
    step for step (iteration counts equal but for round-off at the exit threshold, x to 1e-8);
    qp_init 1 (default): the scaled start, the same optimum to the QP tolerance in fewer or equal
    iterations."""
    cases = load_golden("qp_random.json")["cases"]
    groups = {}
    for cs in cases:
        groups.setdefault((cs["N"], cs["C"]), []).append(cs)
    for (N, C), cl in groups.items():
        s = solver(N, C, use_nlp=0, qp_init=qp_init)
        x0 = np.array([c["x0"] for c in cl]); ref = np.array([c["ref"] for c in cl]); foot = np.array([c["foot"] for c in cl])
        out = s.solve(x0, ref, foot, qp_only=True)
        xr = np.array([c["x"] for c in cl])
        assert (out["status"][:, 0] == 0).all()
        it_ref = np.array([c["iters"] for c in cl])
        if qp_init == 1:
            assert out["iters"][:, 0].mean() <= it_ref.mean()
            np.testing.assert_allclose(xus(N, out["x"]), xus(N, xr), atol=1e-7, rtol=0)
            if C == 2:
                np.testing.assert_allclose(out["x"], xr, atol=QP_TOL, rtol=0)
            continue
        same = out["iters"][:, 0] == it_ref
        # the exit test sits on iSWIFT's 1e-6 residual threshold: round-off may move one
        # instance across it by a single iteration (seen for 4 contacts, non-unique lambda)
        assert np.abs(out["iters"][:, 0] - it_ref).max() <= 1 and same.mean() >= 0.75
        np.testing.assert_allclose(xus(N, out["x"]), xus(N, xr), atol=QP_TOL, rtol=0)
        assert np.abs(xus(N, out["x"][same]) - xus(N, xr[same])).max() < 1e-8
        if C == 2:
            np.testing.assert_allclose(out["x"], xr, atol=QP_TOL, rtol=0)


def test_nlp_random_vs_certified_goldens():
    cases = load_golden("nlp_random.json")["cases"]
    N, C = cases[0]["N"], cases[0]["C"]
    s = solver(N, C, K_obs=cases[0]["K_obs"])
    obstacles = np.asarray(cases[0]["obstacles"])
    x0 = np.array([c["x0"] for c in cases]); ref = np.array([c["ref"] for c in cases]); foot = np.array([c["foot"] for c in cases])
    out = s.solve(x0, ref, foot, obstacles)
    xr = np.array([c["x"] for c in cases])
    assert converged(out["status"]).all()
    np.testing.assert_array_equal(out["iters"][:, 1], [c["iters"] for c in cases])
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, xr), atol=NLP_TOL, rtol=0)
    np.testing.assert_allclose(out["x"], xr, atol=1e-6, rtol=0)
    np.testing.assert_allclose(out["obj"], [c["obj"] for c in cases], atol=1e-6, rtol=0)


# ----------------------------------------------------------------------------- vs oracle
CONFIGS = [
    # N, C, K_obs, K_nbr, agents, use_nlp
    (4, 4, 1, 0, 16, 1),      # reference mode (run_NMPC as written)
    (4, 2, 1, 0, 16, 1),      # reference mode, trot domain
    (10, 2, 3, 0, 64, 1),     # BASELINE configs[1]
    (10, 2, 3, 8, 96, 1),     # configs[2] shape (inter-agent rows), small batch
    (10, 2, 3, 8, 512, 1),    # configs[2] shape on more agents than CUs: the compiled-shape instance 12_4_1_10_2_11
    (20, 2, 3, 0, 24, 1),     # horizon 20
    (10, 4, 3, 0, 16, 1),     # standing, 4 contacts
    (10, 2, 0, 0, 32, 1),     # no obstacles: velocity rows only
]


@pytest.mark.parametrize("N,C,Ko,Kn,A,nlp", CONFIGS)
def test_gpu_matches_oracle(N, C, Ko, Kn, A, nlp):
    b = workload.make_batch(A, N, C, seed=7 * N + C + Kn)
    s = solver(N, C, Ko, Kn, nlp)
    out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    if A == 512:                                # the line of CONFIGS that names its instance: one wave, fused polish
        assert s.waves() == 1 and s.last_kernels() == ("srb_nmpc_kernel_12_4_1_10_2_11", ""), s.last_kernels()
    r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=nlp), b["x0"], b["ref"], b["foot"],
                           b["obstacles"], b["nbr_state"], nthreads=8)
    bad = np.where((conv(out["status"]) != conv(r["status"])).any(1))[0]
    assert bad.size == 0, [(int(a), out["status"][a].tolist(), r["status"][a].tolist(), out["iters"][a].tolist(),
                            r["iters"][a].tolist()) for a in bad]
    # iteration counts: identical except where round-off moves an instance across an exit
    # threshold (one iteration either way)
    assert np.mean(np.all(out["iters"] == r["iters"], 1)) >= 0.85
    assert np.abs(out["iters"] - r["iters"]).max() <= 2
    np.testing.assert_allclose(xus(N, out["x_qp"]), xus(N, r["x_qp"]), atol=QP_TOL, rtol=0)
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)
    if C == 2:
        np.testing.assert_allclose(out["x"], r["x"], atol=NLP_TOL, rtol=0)
    np.testing.assert_allclose(out["obj"], r["obj"], rtol=1e-7, atol=1e-6)


def test_free_velocity_workload_statuses_and_solutions_vs_oracle():
    """The hard workload (workload.make_batch velocity="free": U[-0.3, 0.3] per axis, uncorrelated
    with the goal and the trot support): a few percent of the instances have infeasible CoM-CoP
    rows.  Their duals diverge; both the kernel and the oracle end such a stage FATAL once a dual
    passes SRB_Z_DIV = 1e10 (converging solves stay below ~1e4), at a finite iterate.  So every
    output is finite, the status arrays equal the oracle's, and wherever both are OPTIMAL the
    solutions agree as on the easy workload.  (The reference returns a finite last iterate on a
    non-optimal exit: iswift_qp.cpp:126-151.)"""
    N, C, Ko, Kn, A = 10, 2, 3, 8, 512
    b = workload.make_batch(A, N, C, seed=5, velocity="free")
    s = solver(N, C, Ko, Kn, 1)
    buf = np.zeros((A, 4)); buf[:, 0] = b["x0"][:, 0]; buf[:, 2] = b["x0"][:, 2]
    out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], alpha_buf=buf)
    r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn), b["x0"], b["ref"], b["foot"], b["obstacles"],
                           b["nbr_state"], nthreads=8)
    assert np.isin(out["status"], [0, 1, 2, 3, 4]).all()
    for k in ("x", "x_qp", "obj", "alpha"):                      # every agent, FATAL ones included
        assert np.isfinite(out[k]).all(), (k, np.where(~np.isfinite(out[k]).reshape(A, -1).all(1))[0])
    nonopt = (r["status"] != 0).any(1)
    assert nonopt.sum() >= 5, nonopt.sum()                       # the workload is hard: some fail in both
    diff = np.where((out["status"] != r["status"]).any(1))[0]
    assert diff.size == 0, [(int(a), out["status"][a].tolist(), r["status"][a].tolist()) for a in diff]
    ok_g, ok_o = ok_elem(out["status"]), ok_elem(r["status"])
    assert (ok_g[:, 0] == ok_o[:, 0]).mean() >= 0.99
    assert (ok_g.all(1) == ok_o.all(1)).mean() >= 0.98, (ok_g.all(1) != ok_o.all(1)).sum()
    both = ok_g.all(1) & ok_o.all(1)
    assert both.mean() >= 0.9
    np.testing.assert_allclose(xus(N, out["x_qp"][both]), xus(N, r["x_qp"][both]), atol=QP_TOL, rtol=0)
    np.testing.assert_allclose(xus(N, out["x"][both]), xus(N, r["x"][both]), atol=NLP_TOL, rtol=0)


@pytest.mark.parametrize("N,C", [(4, 4), (4, 2), (10, 2), (10, 4), (20, 2)])
def test_hip_qp_stage_vs_iswift_min_degree_goldens(N, C):
    """the HIP QP stage itself on all 64 instances per (N, C) of
    tests/golden/qp_iswift_md.npz (genuine iSWIFT under a minimum-degree ordering, the stand-in for
    the reference's Eigen AMD, iswift_qp.cpp:184-210): within 1e-7 of each instance's exact optimum
    in X, U, s and never worse than iSWIFT-md in the exact l1 merit -- the checks
    tests/test_oracle.py applies to the oracle, here on the kernel's own output."""
    import os
    from kkt import l1_merit, qp_exact_optimum
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "qp_iswift_md.npz"), allow_pickle=False)
    k = f"N{N}_C{C}_"
    x0, ref, foot = g[k + "x0"], g[k + "ref"], g[k + "foot"]
    out = solver(N, C, use_nlp=0).solve(x0, ref, foot, qp_only=True)
    assert (out["status"][:, 0] == 0).all(), out["status"][:, 0]
    p = oracle.params(N, C)
    sel = np.r_[0:6 * N, -1]
    for a in range(x0.shape[0]):
        Pd, c, A, b, G, h = oracle.build_qp(p, x0[a], ref[a], foot[a])
        x = out["x_qp"][a]
        xs, y, z = qp_exact_optimum(Pd, c, A, b, G, h, g[k + "x_orc"][a])
        fstar = 0.5 * Pd @ (xs * xs) + c @ xs
        assert np.abs(x[sel] - xs[sel]).max() < 1e-7, (a, np.abs(x[sel] - xs[sel]).max())
        m_gpu = l1_merit(Pd, c, A, b, G, h, x, y, z)
        m_md = l1_merit(Pd, c, A, b, G, h, g[k + "x_md"][a], y, z)
        assert m_gpu <= m_md + 1e-12 * max(1.0, abs(fstar)), (a, m_gpu - fstar, m_md - fstar)


# ----------------------------------------------------------------------------- full-size properties
def _dynamics_residual(p, x0, x):
    Ad, Bd = oracle.lip(oracle.params(p.N, p.C))
    N = p.N
    X = x[:, :4 * N].reshape(-1, N, 4); U = x[:, 4 * N:6 * N].reshape(-1, N, 2)
    prev = x0
    err = 0.0
    for k in range(N):
        pred = prev @ Ad.T + U[:, k] @ Bd.T
        err = max(err, np.abs(pred - X[:, k]).max())
        prev = X[:, k]
    return err


@pytest.mark.parametrize("A,Kn", [(64, 0), (1024, 8)])
def test_full_size_properties(A, Kn):
    """BASELINE configs[1] and configs[2] at full size: size-independent properties."""
    N, C, Ko = 10, 2, 3
    b = workload.make_batch(A, N, C, seed=11)
    s = solver(N, C, Ko, Kn)
    out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    p = s.params
    assert converged(out["status"]).mean() >= 0.999            # converged (NLP polished: OPTIMAL) on both stages
    x = out["x"]
    assert _dynamics_residual(p, b["x0"], x) < 1e-9                          # Aeq x = beq (dynamics)
    Xs, U, L, sl = srbnmpc.split(p, x)
    np.testing.assert_allclose(L.sum(-1), 1.0, atol=1e-9)                      # sum lambda = 1
    np.testing.assert_allclose(U, np.einsum("akdc,akc->akd", b["foot"], L), atol=1e-9)   # u = F lambda
    assert L.min() > -1e-7 and L.max() < 1 + 1e-7
    fr = p.mu * p.hcom / np.sqrt(2)
    com_cop = np.abs(Xs[:, :-1][..., [0, 2]] - U[:, 1:])
    assert com_cop.max() < fr + 1e-6
    assert np.abs(Xs[..., [1, 3]]).max() < p.vsat + 1e-6                        # velocity rows
    # obstacle / inter-agent rows: d^2 + s >= eps
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    rng = np.random.default_rng(0)
    for a in rng.choice(A, size=min(A, 24), replace=False):
        obs, eps = oracle.select_obstacles(op, b["x0"][a], b["obstacles"], b["nbr_state"], int(a))
        d2 = ((Xs[a][:, None, [0, 2]] - obs) ** 2).sum(-1)
        assert (d2 + sl[a] - eps[None, :]).min() > -1e-6
        Pd, c, Aeq, beq, G, h = oracle.build_qp(op, b["x0"][a], b["ref"][a], b["foot"][a])
        gJ, hh = nlp_rows(N, C, Pd.size, G, h, obs, eps, p.vsat)
        cert = certify(Pd, c, Aeq, beq, gJ, hh, x[a])
        assert cert["stat_rel"] < 1e-5 and cert["prim"] < 1e-6, (a, cert)


def test_unpolished_loosened_exit_is_acceptable_not_optimal():
    """the NLP stage exits on dual-residual / complementarity tests 10x looser than the
    QP's (SRB_NLP_EXITF) because the polish makes the result exact.  A result that met only those
    loosened tests is provisional: with the polish off (SRB_OPT_POLISH = 0) it must read ACCEPTABLE
    (4), never OPTIMAL, exactly as the oracle with orc_params.polish = 0 says; with the polish on every such
    solve is promoted to OPTIMAL at the exact KKT point."""
    N, C, Ko, Kn, A = 10, 2, 3, 8, 256
    b = workload.make_batch(A, N, C, seed=11)
    p = srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn)
    s = srbnmpc.BatchSolver(p, A)
    try:
        s.set_option("polish", 0)
        assert s.get_option("polish") == 0.0
        off = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
        s.set_option("polish", 1)
        on = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    finally:
        s.close()
    r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn, polish=0), b["x0"], b["ref"], b["foot"],
                           b["obstacles"], b["nbr_state"], nthreads=8)
    prov = off["status"][:, 1] == 4
    assert prov.sum() >= A // 10, prov.sum()                    # the loosened exit is the common case
    assert ((off["status"] == r["status"]).all(1)).mean() >= 0.99
    assert not ((off["status"][:, 1] == 0) & (r["status"][:, 1] == 4)).any()
    assert converged(on["status"]).all()                        # polished: OPTIMAL
    # the interior-point results themselves are unchanged by the status rule
    np.testing.assert_allclose(xus(N, off["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


def test_fused_polish_equals_separate_polish_kernel():
    """the active-set polish runs at the end of the solve kernel
    (SRB_OPT_POLISH_FUSED = 1, default, instances up to NZL 16) instead of as srb_polish_kernel.
    Same algorithm from the same float z snapshot, so the results agree to round-off (the two
    kernels run at different waves per agent, so the reduction orders differ) and every status
    is identical; both match the oracle at NLP_TOL."""
    # (10, 4): nz = N (C - 1) + 1 = 31 > 16, an instance that does not fuse: both launches use the kernel
    for (N, C, Ko, Kn, A, seed, fuses) in [(10, 2, 3, 8, 1024, 5, True), (10, 4, 1, 0, 256, 6, False)]:
        b = workload.make_batch(A, N, C, seed=seed)
        p = srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn)
        s = srbnmpc.BatchSolver(p, A)
        try:
            assert s.get_option("polish_fused") == 1.0
            fu = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
            if fuses:
                assert s.get_option("last_polish") == 2.0 and s.last_polish_ms() == 0.0
            else:
                assert s.get_option("last_polish") == 1.0
            s.set_option("polish_fused", 0)
            se = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
            assert s.get_option("last_polish") == 1.0
        finally:
            s.close()
        np.testing.assert_array_equal(fu["status"], se["status"])
        np.testing.assert_allclose(fu["x"], se["x"], atol=1e-8, rtol=0)
        np.testing.assert_allclose(fu["obj"], se["obj"], rtol=1e-12, atol=1e-9)
        assert (fu["status"][:, 1] == 0).mean() >= 0.99
        r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn), b["x0"][:128], b["ref"][:128],
                               b["foot"][:128], b["obstacles"], b["nbr_state"], nthreads=8)
        np.testing.assert_allclose(xus(N, fu["x"][:128]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


def test_timing_option_changes_nothing_but_the_events():
    """SRB_OPT_TIMING = 0 (bench.py's timed loop): no HIP events around the kernels, so the kernel
    times are unavailable, and the results are bit-identical to a timed launch."""
    N, C, Ko, Kn, A = 10, 2, 3, 8, 256
    b = workload.make_batch(A, N, C, seed=9)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        on = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
        assert s.last_kernel_ms()[1] > 0.0
        s.set_option("timing", 0)
        assert s.get_option("timing") == 0.0
        off = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
        with pytest.raises(RuntimeError):
            s.last_kernel_ms()
    finally:
        s.close()
    for k in ("x", "obj", "status", "iters"):
        np.testing.assert_array_equal(on[k], off[k])


def test_config5_full_size_vs_oracle_and_acceptable_exit():
    """bench config 5 (2048 agents, N = 20, 3 static + 8 neighbour rows) at full size, EVERY
    agent within NLP_TOL (1e-4) of the oracle in X, U, s.

    The interior-point exit needs the residual tests AND a last primal step max |ap dx| < 3e-5
    (SRB_NLP_DXTOL); its result is then polished to the exact KKT point of its active set
    (srb_polish_kernel), which ends the solve OPTIMAL.  A polish that is not
    accepted leaves the interior-point result with
    its status (ACCEPTABLE = 4 at the round-off floor; measured 1 of 2048, the oracle 0); every such
    solution, plus a sample of the rest, must pass the KKT certificate."""
    A, N, C, Ko, Kn = 2048, 20, 2, 3, 8
    b = workload.make_batch(A, N, C, seed=1234)
    s = solver(N, C, Ko, Kn)
    out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    st, it = out["status"], out["iters"]
    assert (st[:, 0] == srbnmpc.QP_WARM).all() and np.isin(st[:, 1], [0, srbnmpc.ACCEPTABLE]).all()
    acc = np.where(st[:, 1] == srbnmpc.ACCEPTABLE)[0]
    assert acc.size <= 0.001 * A, acc.size                         # polish accepted on >= 99.9 %
    assert it[:, 1].max() <= 20                                    # no MAXIT tail (measured max 17)
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    r = oracle.solve_batch(op, b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nthreads=16)
    assert np.isin(r["status"][:, 1], [0, 4]).all() and (r["status"][:, 0] == srbnmpc.QP_WARM).all()
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    assert e.max() < NLP_TOL, (int(np.argmax(e)), float(e.max()))
    both = (st[:, 1] == 0) & (r["status"][:, 1] == 0)        # polished on both sides: the same KKT point
    assert both.mean() >= 0.999 and e[both].max() < 1e-6, (both.mean(), float(e[both].max()))
    rng = np.random.default_rng(5)
    for a in np.r_[acc[:64], rng.choice(A, 16, replace=False)]:
        obs, eps = oracle.select_obstacles(op, b["x0"][a], b["obstacles"], b["nbr_state"], int(a))
        Pd, c, Aeq, beq, G, h = oracle.build_qp(op, b["x0"][a], b["ref"][a], b["foot"][a])
        gJ, hh = nlp_rows(N, C, Pd.size, G, h, obs, eps, s.params.vsat)
        cert = certify(Pd, c, Aeq, beq, gJ, hh, out["x"][a])
        assert cert["stat_rel"] < 1e-5 and cert["prim"] < 1e-6, (int(a), cert)


def _oracle_sel(op, b, ob, nb, Ko, Kn, offset=0):
    return np.array([oracle.select_idx(op, b["x0"][a], ob, nb, offset + a) for a in range(b["x0"].shape[0])],
                    np.int32).reshape(-1, Ko + Kn)


@pytest.mark.parametrize("Ko,Kn", [(0, 8), (3, 0), (2, 12)])
def test_knn_matches_bruteforce(Ko, Kn):
    """Obstacle / neighbour selection (srb_knn_kernel; its insertion network is 4, 8 or 16 deep
    by K): the selected indices == the reference's scan order (MPC_dist.cpp:371-382: sqrt
    distance, lower index on ties) for every agent, ties included -- exact ties at different
    positions (so the choice changes the constraint) and sqrt-rounding ties."""
    from test_oracle import sqrt_tie_pair
    N, C, A = 10, 2, 512
    b = workload.make_batch(A, N, C, seed=3)
    rng = np.random.default_rng(8)
    nb = b["nbr_state"].copy()
    ob = b["obstacles"].copy()
    # agents 0..7 at exact coordinates with exact-distance ties at mirrored positions
    for a in range(8):
        # translate agent a's whole problem (state, reference, footholds) to the nearest
        # quarter-metre point, where the mirrored offsets below give bit-equal distances
        px, py = np.round(b["x0"][a, [0, 2]] * 4) / 4
        dx, dy = px - b["x0"][a, 0], py - b["x0"][a, 2]
        b["x0"][a, 0] += dx; b["x0"][a, 2] += dy
        b["x0"][a, [0, 2]] = (px, py); nb[a, :2] = (px, py)
        b["ref"][a, 0::4] += dx; b["ref"][a, 2::4] += dy
        b["foot"][a, :, 0] += dx; b["foot"][a, :, 1] += dy
        # (clearances d^2 = 3.25 and 7.3125 stay above eps = 1.9 / 2.2: feasible instances)
        ob[20 + 2 * a] = (px + 1.5, py + 1.0); ob[21 + 2 * a] = (px - 1.5, py - 1.0)
        nb[100 + 2 * a, :2] = (px - 1.5, py + 2.25); nb[101 + 2 * a, :2] = (px + 1.5, py - 2.25)
    # agents 8..11: sqrt-rounding ties (larger d^2 at the lower index)
    for a in range(8, 12):
        px, py = b["x0"][a, 0], b["x0"][a, 2]
        near, far = sqrt_tie_pair(px, py, rng)
        ob[40 + 2 * a] = far; ob[41 + 2 * a] = near
        near, far = sqrt_tie_pair(px, py, rng)
        nb[130 + 2 * a, :2] = far; nb[131 + 2 * a, :2] = near
    out = solver(N, C, Ko, Kn).solve(b["x0"], b["ref"], b["foot"], ob, nb)
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    np.testing.assert_array_equal(out["sel"], _oracle_sel(op, b, ob, nb, Ko, Kn))
    r = oracle.solve_batch(op, b["x0"], b["ref"], b["foot"], ob, nb, nthreads=8)
    np.testing.assert_array_equal(conv(out["status"]), conv(r["status"]))
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


@pytest.mark.parametrize("n_tab", [5, 64, 256, 257, 1024, 1025, 2048, 2049, 5000])
def test_knn_threshold_pass_table_sizes(n_tab):
    """Round 6's thresholded scan (srb_knn.h knn_thresh: 4, 16 or 32 register slots a lane by the table's size,
    the batched scan beyond 2048 rows) at every size boundary, through srb_select_device on one table and on both
    (one wave each): the reference's order exactly (oracle.select_idx) -- with exact-distance ties (a table
    snapped to a quarter-metre lattice around lattice-aligned agents), NaN rows, the agent's own row, and K
    larger than the rows within reach."""
    rng = np.random.default_rng(n_tab)
    N, C, A = 10, 2, min(96, n_tab)                   # (the batch's agents are rows of the snapshot)
    b = workload.make_batch(A, N, C, seed=40 + n_tab % 7)
    x0 = b["x0"].copy()
    x0[:, [0, 2]] = np.round(x0[:, [0, 2]] * 4) / 4
    half = max(4.0, 0.5 * np.sqrt(n_tab))
    tab = np.zeros((n_tab, 4))
    tab[:, :2] = np.round(rng.uniform(-half, half, (n_tab, 2)) * 4) / 4 + x0[rng.integers(0, A, n_tab)][:, [0, 2]]
    tab[:, 2:] = rng.normal(0, 0.2, (n_tab, 2))
    off = int(rng.integers(0, n_tab - A + 1))
    tab[off:off + A, 0] = x0[:, 0]; tab[off:off + A, 1] = x0[:, 2]   # the agents' own rows
    nan_rows = np.setdiff1d(rng.choice(n_tab, max(1, n_tab // 50), replace=False), np.arange(off, off + A))
    tab[nan_rows, :2] = np.nan                         # (never an agent's own row)
    obs = tab[:, :2].copy()
    dev = torch.device("cuda:0")
    T = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    for Ko, Kn in ((3, 0), (0, 8), (16, 0), (3, 8), (2, 12), (2, 4)):
        if Ko > n_tab or Kn > n_tab - 1:
            continue                                   # (tables shorter than K: test_knn_sentinel_and_missing_rows)
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
        ko, kn = s.n_selected(n_tab, n_tab)
        sel = torch.full((A, ko + kn), -7, dtype=torch.int32, device=dev)
        tables = (1 if Ko else 0) | (2 if Kn else 0)
        s.select_device(T(x0), T(obs), T(tab), sel, tables=tables, agent_offset=off,
                        stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        got = sel.cpu().numpy()
        s.close()
        op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
        want = np.array([oracle.select_idx(op, x0[a], obs, tab, off + a) for a in range(A)], np.int32).reshape(A, -1)
        np.testing.assert_array_equal(got, want, err_msg=f"n_tab {n_tab} K {Ko}+{Kn}")


@pytest.mark.parametrize("Ko,Kn", [(3, 8), (16, 16)])
def test_knn_grid_matches_bruteforce(Ko, Kn):
    """Tables of SRB_GRID_MIN_ROWS (8192) rows or more go through the uniform selection grid
    (srb_grid_build_kernel + the ring search of knn_select_k): the selected rows must be the
    reference's scan order exactly -- exact-distance ties, sqrt-rounding ties, NaN rows, a
    shard offset, and agents far outside the grid (brute-force fallback) included."""
    from test_oracle import sqrt_tie_pair
    N, C, A, n_nbr, n_obs, off = 10, 2, 384, 9000, 12000, 512
    rng = np.random.default_rng(21)
    b = workload.make_batch(A, N, C, seed=5)
    big = workload.make_batch(n_nbr, N, C, seed=6, n_obs=n_obs)
    nb = big["nbr_state"].copy(); ob = big["obstacles"].copy()
    nb[off:off + A] = b["nbr_state"]                     # this shard's agents at rows off..off+A
    # agents 0..7: exact ties at mirrored positions around a quarter-metre-aligned agent
    for a in range(8):
        px, py = np.round(b["x0"][a, [0, 2]] * 4) / 4
        dx, dy = px - b["x0"][a, 0], py - b["x0"][a, 2]
        b["x0"][a, [0, 2]] = (px, py); nb[off + a, :2] = (px, py)
        b["ref"][a, 0::4] += dx; b["ref"][a, 2::4] += dy
        b["foot"][a, :, 0] += dx; b["foot"][a, :, 1] += dy
        ob[20 + 2 * a] = (px + 1.5, py + 1.0); ob[21 + 2 * a] = (px - 1.5, py - 1.0)
        nb[9 + 2 * a, :2] = (px - 1.5, py + 2.25); nb[10 + 2 * a, :2] = (px + 1.5, py - 2.25)
    for a in range(8, 12):                                 # sqrt-rounding ties
        px, py = b["x0"][a, 0], b["x0"][a, 2]
        near, far = sqrt_tie_pair(px, py, rng); ob[60 + 2 * a] = far; ob[61 + 2 * a] = near
        near, far = sqrt_tie_pair(px, py, rng); nb[40 + 2 * a, :2] = far; nb[41 + 2 * a, :2] = near
    nb[100:140, :2] = np.nan; ob[100:140] = np.nan          # rows outside every cell
    b["x0"][20, [0, 2]] = (5000.0, -4000.0)                # far outside the grid: brute-force fallback
    nb[off + 20, :2] = (5000.0, -4000.0)
    out = solver(N, C, Ko, Kn).solve(b["x0"], b["ref"], b["foot"], ob, nb, agent_offset=off)
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    want = np.array([oracle.select_idx(op, b["x0"][a], ob, nb, off + a) for a in range(A)], np.int32)
    np.testing.assert_array_equal(out["sel"], want)


@pytest.mark.parametrize("n_obs", [10000, 5120])
def test_knn_grid_obstacle_version_reuse(n_obs):
    """obstacles_version: an unchanged obstacle table keeps its selection grid across calls; a
    new version rebuilds it (device API).  5120 rows: a versioned table of fewer than
    SRB_GRID_MIN_ROWS rows still gets the grid (SRB_GRID_MIN_ROWS_STATIC), version 0 the scan."""
    N, C, A = 10, 2, 256
    b = workload.make_batch(A, N, C, seed=8)
    ob1 = workload.make_batch(4 * n_obs // 20, N, C, seed=9, n_obs=n_obs)["obstacles"]
    ob2 = ob1[::-1].copy()
    s = solver(N, C, 3, 0)
    dev = torch.device("cuda:0")
    T = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    x0, ref, foot, tob = T(b["x0"]), T(b["ref"]), T(b["foot"].reshape(A, -1)), T(ob1)
    op = oracle.params(N, C, K_obs=3)
    sels = []
    for ver, table in ((1, ob1), (1, ob1), (2, ob2), (0, ob1)):
        tob.copy_(T(table))
        o = dict(x_qp=None, x=torch.zeros((A, s.params.nv), dtype=torch.float64, device=dev),
                 obj=torch.zeros(A, dtype=torch.float64, device=dev), status=torch.zeros((A, 2), dtype=torch.int32, device=dev),
                 iters=torch.zeros((A, 2), dtype=torch.int32, device=dev), sel=torch.zeros((A, 3), dtype=torch.int32, device=dev))
        s.solve_device(x0, ref, foot, tob, None, o, obstacles_version=ver)
        torch.cuda.synchronize()
        sel = o["sel"].cpu().numpy()
        want = np.array([oracle.select_idx(op, b["x0"][a], table) for a in range(A)], np.int32)
        np.testing.assert_array_equal(sel, want)
        sels.append(sel)


def test_knn_sentinel_and_missing_rows():
    """The reference's min_dist = 1000 / min_i = 0 start (MPC_dist.cpp:371-372): with no
    static obstacle closer than 1000 m every static round selects obstacle 0; a neighbour
    table with fewer finite rows than K_nbr leaves -1 slots, whose rows sit 1000 m from the
    agent (as in the oracle), and the solve does not read unwritten LDS."""
    N, C, A, Ko, Kn = 10, 2, 32, 2, 4
    b = workload.make_batch(A, N, C, seed=12)
    ob = np.array([[2500.0, 0.0], [0.0, -1200.0], [1001.0, 1001.0]])
    nb = b["nbr_state"].copy()
    nb[3:, :2] = np.nan                                       # only agents 0..2 are finite
    nb[:3] = b["nbr_state"][:3]
    out = solver(N, C, Ko, Kn).solve(b["x0"], b["ref"], b["foot"], ob, nb)
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    want = _oracle_sel(op, b, ob, nb, Ko, Kn)
    np.testing.assert_array_equal(out["sel"], want)
    # agents 3.. see the three finite rows 0..2, agents 0..2 the other two
    assert (out["sel"][:, :Ko] == 0).all() and (out["sel"][3:, Ko + 3] == -1).all()
    assert (out["sel"][:3, Ko + 2:] == -1).all() and (out["sel"][3:, Ko:Ko + 3] >= 0).all()
    r = oracle.solve_batch(op, b["x0"], b["ref"], b["foot"], ob, nb, nthreads=8)
    np.testing.assert_array_equal(conv(out["status"]), conv(r["status"]))
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


@pytest.mark.parametrize("shards,nw", [(2, 0), (8, 1), (8, 4)])
def test_sharded_solve_matches_full_batch(shards, nw):
    """The multi-GPU data path on one GPU: each shard is what one rank solves after the
    all-gather (srbnmpc.dist): its contiguous agent block with agent_offset = lo and the FULL
    neighbour table (MPC_dist.cpp:1272-1276 rows of every agent).  Statuses, x and the
    selected rows are bit-identical to the single-batch solve with the same waves per agent
    (nw; 0 = the automatic choice, the same for 512- and 1024-agent batches), which matches
    the oracle."""
    from srbnmpc import dist as sdist
    N, C, A, Ko, Kn = 10, 2, 1024, 3, 8
    b = workload.make_batch(A, N, C, seed=77)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    s.set_waves(nw)
    full = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    nw_full = s.waves()
    dev = torch.device("cuda:0")
    T = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    nbr = T(b["nbr_state"]); obst = T(b["obstacles"])
    parts, keep = [], []
    for r in range(shards):
        lo, hi = sdist.shard_range(A, shards, r)
        n = hi - lo
        ins = (T(b["x0"][lo:hi]), T(b["ref"][lo:hi]), T(b["foot"][lo:hi].reshape(n, -1)))
        keep.append(ins)                      # inputs stay allocated until the launches have run
        o = dict(x_qp=None, x=torch.zeros((n, s.params.nv), dtype=torch.float64, device=dev),
                 obj=torch.zeros(n, dtype=torch.float64, device=dev),
                 status=torch.zeros((n, 2), dtype=torch.int32, device=dev),
                 iters=torch.zeros((n, 2), dtype=torch.int32, device=dev),
                 sel=torch.full((n, Ko + Kn), -2, dtype=torch.int32, device=dev))
        s.solve_device(*ins, obst, nbr, o, agent_offset=lo)
        parts.append(o)
    torch.cuda.synchronize()
    assert s.waves() == nw_full
    s.close()
    cat = {k: np.concatenate([o[k].cpu().numpy() for o in parts]) for k in ("x", "obj", "status", "iters", "sel")}
    bad = np.where((cat["status"] != full["status"]).any(1) | (cat["x"] != full["x"]).any(1))[0]
    assert bad.size == 0, (bad[:10], cat["status"][bad[:5]], full["status"][bad[:5]])
    for k in cat:
        np.testing.assert_array_equal(cat[k], full[k], err_msg=k)
    # the shard rows exclude their own global index from the neighbours
    assert not np.any(cat["sel"][:, Ko:] == np.arange(A)[:, None])
    r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn), b["x0"], b["ref"], b["foot"], b["obstacles"],
                           b["nbr_state"], nthreads=16)
    np.testing.assert_array_equal(conv(cat["status"]), conv(r["status"]))
    np.testing.assert_allclose(xus(N, cat["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


def test_qp_only_equals_qp_stage():
    """srb_solve_qp (use_nlp = 0) runs the QP to the full tolerance: bit-identical to the QP stage of a full
    solve with SRB_OPT_QP_WARM_TOL = 0."""
    N, C = 10, 2
    b = workload.make_batch(32, N, C, seed=21)
    full = solver(N, C, 3, 0, 1, qp_warm_tol=0.0).solve(b["x0"], b["ref"], b["foot"], b["obstacles"])
    qp = solver(N, C, 3, 0, 0).solve(b["x0"], b["ref"], b["foot"], b["obstacles"], qp_only=True)
    np.testing.assert_array_equal(qp["x"], full["x_qp"])
    assert (qp["iters"][:, 1] == 0).all()


def _warm_workload(name):
    if name == "c3":
        A, b, _, _ = bench.rank_batch(3, 1024, 1, 0)
        cfg = bench.CONFIGS[3]
        return cfg["N"], cfg["C"], cfg["K_obs"], cfg["K_nbr"], b
    if name == "c5":
        A, b, _, _ = bench.rank_batch(5, 2048, 1, 0)
        cfg = bench.CONFIGS[5]
        return cfg["N"], cfg["C"], cfg["K_obs"], cfg["K_nbr"], b
    if name == "free":                       # infeasible and near-infeasible instances (FATAL in both)
        return 10, 2, 3, 8, workload.make_batch(512, 10, 2, seed=0, velocity="free")
    # crowded: four times the obstacle density of the reference's arena
    return 10, 2, 3, 8, workload.make_batch(1024, 10, 2, seed=5, n_obs=int(round(80 * workload.arena_scale(1024) ** 2)))


@pytest.mark.parametrize("name", ["c3", "free", "dense", "c5"])
def test_qp_warm_tolerance_leaves_the_nlp_result(name):
    """SRB_OPT_QP_WARM_TOL (default 0.3): the QP stage only warm-starts the NLP
    (MPC_dist.cpp:403 starts SNOPT from iSWIFT's point), so stopping it early must leave the NLP's statuses
    unchanged and its result within the polish's step tolerance (1e-7) -- on the configs[2] batch, the hard
    free-velocity workload, a crowded arena and config 5 (N = 20), the kernel at 0.3 against the kernel at 0
    (the full 1e-6).  A warm QP stage reports QP_WARM (4), never OPTIMAL.  The oracle makes the same
    comparison on the CPU (tests/test_oracle.py::test_oracle_qp_warm_tolerance_leaves_the_nlp_result)."""
    N, C, Ko, Kn, b = _warm_workload(name)
    args = (b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    s = solver(N, C, Ko, Kn)
    assert s.get_option("qp_warm_tol") == 3e-1
    warm = s.solve(*args)
    full = solver(N, C, Ko, Kn, qp_warm_tol=0.0).solve(*args)
    np.testing.assert_array_equal(warm["status"][:, 1], full["status"][:, 1])
    np.testing.assert_array_equal(ok_elem(warm["status"])[:, 0], ok_elem(full["status"])[:, 0])
    assert not (warm["status"][:, 0] == 0).any() and not (full["status"][:, 0] == srbnmpc.QP_WARM).any()
    both = warm["status"][:, 1] == 0
    assert both.mean() >= (0.9 if name == "free" else 0.99)
    np.testing.assert_allclose(xus(N, warm["x"][both]), xus(N, full["x"][both]), atol=1e-7, rtol=0)
    assert warm["iters"][:, 0].mean() < full["iters"][:, 0].mean() - 1.0
    if name == "c3":
        assert warm["iters"][:, 0].max() < full["iters"][:, 0].max()
        r = oracle.solve_batch(oracle.params(N, C, K_obs=Ko, K_nbr=Kn), *args, nthreads=16)
        np.testing.assert_array_equal(conv(warm["status"]), conv(r["status"]))
        assert (warm["iters"][:, 0] == r["iters"][:, 0]).mean() > 0.95
        np.testing.assert_allclose(xus(N, warm["x"]), xus(N, r["x"]), atol=NLP_TOL, rtol=0)


def test_device_api_matches_host():
    N, C, A = 10, 2, 64
    b = workload.make_batch(A, N, C, seed=4)
    s = solver(N, C, 3, 8)
    host = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    dev = torch.device("cuda:0")
    t = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev) for k, v in b.items()}
    out = dict(x_qp=torch.zeros((A, s.params.nv), dtype=torch.float64, device=dev),
               x=torch.zeros((A, s.params.nv), dtype=torch.float64, device=dev),
               obj=torch.zeros(A, dtype=torch.float64, device=dev),
               status=torch.zeros((A, 2), dtype=torch.int32, device=dev),
               iters=torch.zeros((A, 2), dtype=torch.int32, device=dev))
    s.solve_device(t["x0"], t["ref"], t["foot"].reshape(A, -1), t["obstacles"], t["nbr_state"], out,
                   stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.current_stream(dev).synchronize()
    np.testing.assert_array_equal(out["x"].cpu().numpy(), host["x"])
    np.testing.assert_array_equal(out["status"].cpu().numpy(), host["status"])


@pytest.mark.parametrize("world,rank", [(1, 0), (8, 3)])
def test_split_selection_around_the_collective_equals_one_pass(world, rank):
    """bench.py's multi-GPU step: the static obstacles selected on the compute
    stream while the neighbour all-gather is in flight (srb_select_device, tables 1), the neighbours after it
    (tables 2, ordered by the collective's wait), then the solve with SRB_OPT_SELECTION = 0 -- bit-identical to
    the solve's own one-pass selection (sel, x, status), for a single GPU and rank 3 of an 8-GPU configs[3]
    swarm (its agent_offset, the whole snapshot)."""
    A_total, b, lo, hi = bench.rank_batch(3, 1024 // world if world > 1 else 256, world, rank)
    N, C, Ko, Kn = 10, 2, 3, 8
    dev = torch.device("cuda:0")
    t = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev) for k, v in b.items()}
    x0, ref, foot = t["x0"][lo:hi].contiguous(), t["ref"][lo:hi].contiguous(), t["foot"][lo:hi].reshape(hi - lo, -1).contiguous()
    A = hi - lo
    res = {}
    for mode in ("one", "split"):
        s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
        ko, kn = s.n_selected(t["obstacles"].shape[0], A_total)
        out = dict(x_qp=None, x=torch.zeros((A, s.params.nv), dtype=torch.float64, device=dev),
                   obj=torch.zeros(A, dtype=torch.float64, device=dev),
                   status=torch.zeros((A, 2), dtype=torch.int32, device=dev),
                   iters=torch.zeros((A, 2), dtype=torch.int32, device=dev),
                   sel=torch.full((A, ko + kn), -7, dtype=torch.int32, device=dev))
        st = torch.cuda.current_stream(dev).cuda_stream
        if mode == "split":
            side = torch.cuda.Stream(dev)
            s.select_device(x0, t["obstacles"], t["nbr_state"], out["sel"], tables=1, agent_offset=lo, stream=st)
            ev = torch.cuda.Event()
            with torch.cuda.stream(side):             # stands in for the RCCL stream of the all-gather
                nb = t["nbr_state"].clone()
                ev.record(side)
            torch.cuda.current_stream(dev).wait_event(ev)
            s.select_device(x0, t["obstacles"], nb, out["sel"], tables=2, agent_offset=lo, stream=st)
            s.set_option("selection", 0)
        else:
            nb = t["nbr_state"]
        s.solve_device(x0, ref, foot, t["obstacles"], nb, out, agent_offset=lo, stream=st)
        torch.cuda.current_stream(dev).synchronize()
        res[mode] = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
        s.close()
    for k in ("sel", "x", "status", "iters", "obj"):
        np.testing.assert_array_equal(res["split"][k], res["one"][k])
    assert (res["one"]["sel"] >= 0).all()


def test_edge_cases():
    N, C = 10, 2
    s = solver(N, C, 3, 0, 1, max_agents=8)
    b = workload.make_batch(8, N, C, seed=9)
    # empty batch is a no-op
    out = s.solve(b["x0"][:0], b["ref"][:0], b["foot"][:0], b["obstacles"])
    assert out["x"].shape == (0, s.params.nv)
    # more agents than the context holds -> error, not a fault
    with pytest.raises(RuntimeError):
        s.solve(np.tile(b["x0"], (2, 1)), np.tile(b["ref"], (2, 1)), np.tile(b["foot"], (2, 1, 1, 1)), b["obstacles"])
    # fewer obstacles than K_obs: "up to K nearest" (K clamped to what exists, as in the oracle)
    few = b["obstacles"][:1]
    out = s.solve(b["x0"], b["ref"], b["foot"], few)
    r = oracle.solve_batch(oracle.params(N, C, K_obs=3), b["x0"], b["ref"], b["foot"], few)
    np.testing.assert_array_equal(conv(out["status"]), conv(r["status"]))
    np.testing.assert_allclose(xus(N, out["x"]), xus(N, r["x"]), atol=NLP_TOL)
    # identical agents give identical answers (no cross-agent interference in the batch)
    same = s.solve(np.repeat(b["x0"][:1], 8, 0), np.repeat(b["ref"][:1], 8, 0), np.repeat(b["foot"][:1], 8, 0),
                   b["obstacles"])
    assert (same["x"] == same["x"][0]).all()


def test_mpcdist_surface_on_reference_instance(kat2):
    """MPC_dist call sequence (src/A1_Sim.cpp:180-197) through MPCDist on the logged instance."""
    m = srbnmpc.MPCDist()
    m.setAgentID(0)
    m.setPstart(np.zeros(8))
    obst = np.asarray(kat2["obstacle"])
    m.setPobs_real(np.c_[obst, [50.0, 50.0]])
    ref = np.asarray(kat2["ref"]).reshape(4, 4)          # grid-major (x, xdot, y, ydot)
    Pr = np.zeros((8, 8)); Prd = np.zeros((8, 8))
    Pr[0, :4] = ref[:, 0]; Prd[0, :4] = ref[:, 1]; Pr[1, :4] = ref[:, 2]; Prd[1, :4] = ref[:, 3]
    m.setReferenceTrajectory(Pr, Prd)
    q = np.zeros(18); dq = np.zeros(18)
    x0 = kat2["x0"]
    q[0], dq[0], q[1], dq[1] = x0[0], x0[1], x0[2], x0[3]
    m.updateState(q, dq, [1, 1, 1, 1], np.zeros((3, 4)), np.zeros(4))
    m.use_snopt = True
    m.run_NMPC()
    np.testing.assert_allclose(m.get_MPCsol().ravel(), np.asarray(kat2["x_nlp"])[:16], atol=1e-6)
    np.testing.assert_allclose(m.qp_solution_eventbased_[:24], kat2["logged_qp_x"], atol=2e-9)
    alpha = m.get_alphaCOM()
    np.testing.assert_allclose(alpha, oracle.fit_bezier([0, 0, 0, 0], np.asarray(kat2["x_nlp"])[:16].reshape(4, 4)),
                               atol=1e-6)
    assert m.gaitDomain_ == 1


def test_mpcdist_horizon_10_trot_cycles_vs_oracle():
    """BASELINE configs[0]: one A1 agent, horizon 10, trot, through MPCDist(horizon=10) for three
    control cycles (the window advances NDOMAIN = 4 columns a cycle, the predicted state seeds the
    next): statuses, QP point and NLP point against the oracle on the same inputs."""
    N, C = 10, 2
    m = srbnmpc.MPCDist(horizon=N)
    m.setAgentID(0)
    m.setPstart(np.zeros(2))
    Pobs = np.array([[0.9, 0.35], [2.0, -1.0], [3.1, 0.6]])
    m.setPobs_real(Pobs.T)
    T = 40
    c = np.arange(T)
    Pr = np.zeros((2, T)); Prd = np.zeros((2, T))
    Pr[0] = 0.27 * 0.043 * (c + 1); Prd[0] = 0.27
    m.setReferenceTrajectory(Pr, Prd)
    m.use_snopt = True
    p = oracle.params(N, C, K_obs=1, use_nlp=1, tol_qp=0.0)          # MPCDist keeps the full QP tolerance
    q = np.zeros(18); dq = np.zeros(18)
    # moving start (test_cpp_shim's): from rest at the origin the agent sits inside the first
    # obstacle's eps radius and the NLP ends FATAL (dual divergence) there, on the GPU and in the oracle alike
    q[0], dq[0], q[1], dq[1] = 0.02, 0.1, -0.01, 0.02
    for cyc in range(3):
        ind = [1, 0, 0, 1] if cyc % 2 == 0 else [0, 1, 1, 0]          # trot: FR + RL, then FL + RR
        m.updateState(q, dq, ind, m.toePos_, np.zeros(4))
        ref = m.copPlanner_eventbase()
        foot = np.repeat(m.footholdsPlanner()[None], N, 0)
        x0 = np.array([q[0], dq[0], q[1], dq[1]])
        buf = m.mpc_state_alpha_buffer_.copy()
        m.run_NMPC()
        r = oracle.solve_batch(p, x0[None], ref[None], foot[None], Pobs)
        assert m.last_status.tolist() == r["status"][0].tolist() == [0, 0], (cyc, m.last_status, r["status"])
        np.testing.assert_allclose(xus(N, m.qp_solution_eventbased_), xus(N, r["x_qp"][0]), atol=QP_TOL, rtol=0)
        np.testing.assert_allclose(m.get_MPCsol().ravel(), r["x"][0][:4 * N], atol=NLP_TOL, rtol=0)
        X = m.get_MPCsol().reshape(N, 4)
        np.testing.assert_allclose(m.get_alphaCOM(), oracle.fit_bezier(buf, X[:4]), atol=1e-9)
        q[0], dq[0], q[1], dq[1] = X[3]
    assert m.gaitDomain_ == 3 and m.get_MPCsol().shape == (4 * N, 1)


@pytest.mark.parametrize("N,C,Kn", [(4, 4, 0), (10, 2, 8)])
def test_fused_bezier_epilogue_matches_reference_fit(N, C, Kn):
    """fitComTrajectory_eventbase (MPC_dist.cpp:784-855) fused into the solve == the oracle's
    literal 24x24 KKT restatement on the same predicted states and buffer."""
    A = 48
    b = workload.make_batch(A, N, C, seed=31 + N)
    rng = np.random.default_rng(5)
    buf = np.stack([b["x0"][:, 0], rng.uniform(-0.2, 0.2, A), b["x0"][:, 2], rng.uniform(-0.2, 0.2, A)], 1)
    s = solver(N, C, 3, Kn)
    out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], alpha_buf=buf)
    plain = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    np.testing.assert_array_equal(out["x"], plain["x"])          # the epilogue does not touch the solve
    for a in range(A):
        X = out["x"][a, :16].reshape(4, 4)
        want = oracle.fit_bezier(buf[a], X)
        np.testing.assert_allclose(out["alpha"][a], want, rtol=0, atol=1e-10 * max(1.0, np.abs(want).max()))
        np.testing.assert_allclose(out["alpha"][a][:, 0], buf[a], atol=1e-12)   # a_0 = buffer (s = 0 row)
        np.testing.assert_allclose(out["alpha"][a][:, 4], X[3], atol=1e-9)       # a_4 = X_3 (s = 1)


@pytest.mark.parametrize("C", [2, 4])
def test_device_input_assembly_matches_host_planners(C):
    """srb_prepare_batch_device == the reference's copPlanner_eventbase / footholdsPlanner /
    updateState / get_lastState (restated host-side in srbnmpc.MPCDist) for a batch."""
    N, A, NA, T = 4, 40, 40, 64
    rng = np.random.default_rng(17 + C)
    Pr = rng.uniform(-3, 9, (2 * NA, T)); Prd = rng.uniform(-0.4, 0.4, (2 * NA, T))
    gd = rng.integers(0, 10, A).astype(np.int32)
    contact = np.zeros((A, 4), np.int32)
    for a in range(A):
        contact[a] = [1, 1, 1, 1] if C == 4 else ([1, 0, 0, 1] if a % 2 else [0, 1, 1, 0])
    toe = rng.uniform(-1, 9, (A, 3, 4)); start = rng.uniform(0, 9, (A, 2))
    q = rng.normal(size=(A, 18)); dq = rng.normal(size=(A, 18))
    dev = torch.device("cuda:0")
    tt = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    s = solver(N, C, 1, 0, 1, max_agents=64)
    out = dict(x0=torch.zeros((A, 4), dtype=torch.float64, device=dev), ref=torch.zeros((A, 4 * N), dtype=torch.float64, device=dev),
               foot=torch.zeros((A, N * 2 * C), dtype=torch.float64, device=dev),
               last_state=torch.zeros((A, 4), dtype=torch.float64, device=dev), status=torch.full((A,), -1, dtype=torch.int32, device=dev))
    s.prepare_device(tt(Pr.T), tt(Prd.T), tt(gd, torch.int32), tt(contact, torch.int32), tt(toe), tt(start), tt(q), tt(dq), out)
    s.sync()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ok = 4 * gd + N <= T
    np.testing.assert_array_equal(got["status"], np.where(ok, 0, 2))
    for a in range(A):
        m = srbnmpc.MPCDist()
        m.setAgentID(a)
        Ps = np.zeros(2 * NA); Ps[2 * a:2 * a + 2] = start[a]
        m.setPstart(Ps)
        m.setReferenceTrajectory(Pr, Prd)
        m.updateState(q[a], dq[a], contact[a], toe[a], np.zeros(4))
        m.gaitDomain_ = int(gd[a])
        np.testing.assert_array_equal(got["x0"][a], [q[a, 0], dq[a, 0], q[a, 1], dq[a, 1]])
        np.testing.assert_array_equal(got["last_state"][a], m.get_lastState())
        F = m.footholdsPlanner()
        np.testing.assert_array_equal(got["foot"][a].reshape(N, 2, C), np.repeat(F[None], N, 0))
        if ok[a]:
            # window of the current domain: columns 4 gaitDomain_ .. + N (N == NDOMAIN here)
            np.testing.assert_array_equal(got["ref"][a], m.copPlanner_eventbase(N))
    # and the assembled batch solves like the host-assembled one
    good = np.where(ok)[0][:16]
    sub = {k: v[good] for k, v in got.items()}
    obst = rng.uniform(0, 9, (20, 2))
    r1 = s.solve(sub["x0"], sub["ref"], sub["foot"], obst)
    assert (r1["status"] >= 0).all()


@pytest.mark.parametrize("NA,n_obs,loop", [(4, 20, 20000), (64, 40, 4000), (300, 60, 2000)])
def test_hl_planner_bitwise_vs_oracle(NA, n_obs, loop):
    """generateReferenceTrajectory on the device == the CPU restatement, bit for bit (same
    operation order, no contraction); reference start layout for NA = 4."""
    rng = np.random.default_rng(NA)
    if NA == 4:
        Ps = np.array([0.0, 0.0, 0.0, -0.9, -1, 0, -1, -0.9])         # src/A1_Sim.cpp:1013
    else:
        Ps = np.stack([rng.uniform(-4, 0, NA), rng.uniform(-3, 3, NA)], 1).ravel()
    Po = np.stack([rng.uniform(0, 9, n_obs), rng.uniform(-2, 2, n_obs)], 1)
    Pr, Prd = srbnmpc.hl_plan(Ps, Po, loop=loop)
    R, Rd = oracle.hl_plan(Ps, Po, loop=loop)
    assert Pr.shape == (2 * NA, loop // 40)
    np.testing.assert_array_equal(Pr, R)
    np.testing.assert_array_equal(Prd, Rd)


def test_hl_planner_multi_workgroup_swarm_bitwise():
    """A swarm beyond one workgroup (NA = 1100 > 1024): one coupled swarm, one launch per step
    across the chip, still bit-identical to the CPU restatement."""
    NA, n_obs, loop = 1100, 30, 160
    rng = np.random.default_rng(11)
    Ps = np.stack([rng.uniform(-30, 0, NA), rng.uniform(-15, 15, NA)], 1).ravel()
    Po = np.stack([rng.uniform(0, 9, n_obs), rng.uniform(-2, 2, n_obs)], 1)
    Pr, Prd = srbnmpc.hl_plan(Ps, Po, loop=loop)
    R, Rd = oracle.hl_plan(Ps, Po, loop=loop)
    np.testing.assert_array_equal(Pr, R)
    np.testing.assert_array_equal(Prd, Rd)


def test_closed_loop_hl_to_solve_through_mpcdist():
    """A1_Sim.cpp:1152-1156 then :180-197 for several control cycles: the device HL planner
    feeds MPCDist.run_NMPC; every cycle's solve equals the oracle on the same inputs and the
    agent's predicted state seeds the next cycle."""
    Ps = np.array([0.0, 0.0, 0.0, -0.9, -1, 0, -1, -0.9])             # src/A1_Sim.cpp:1013
    Pobs = np.array([[3.0, 0.2], [5.0, -0.6], [7.0, 0.4]])
    m = srbnmpc.MPCDist()
    m.setAgentID(1)
    m.setPstart(Ps)
    m.setPobs(Pobs.T)
    m.setPobs_real(Pobs.T)
    m.generateReferenceTrajectory(loop=4000)
    R, Rd = oracle.hl_plan(Ps, Pobs, loop=4000)
    np.testing.assert_array_equal(m.Pr_refined_, R)
    np.testing.assert_array_equal(m.Prd_refined_, Rd)
    m.use_snopt = True
    p = oracle.params(4, 4, K_obs=1, use_nlp=1, tol_qp=0.0)          # MPCDist keeps the full QP tolerance
    q = np.zeros(18); dq = np.zeros(18)
    q[:2] = Ps[2:4]
    from srbnmpc.mpc_dist import INIT_FOOTPRINT
    for cyc in range(6):
        toe = np.zeros((3, 4))                 # stance around the current CoM (the simulator's toePos)
        toe[0] = INIT_FOOTPRINT[:, 0] + q[0]; toe[1] = INIT_FOOTPRINT[:, 1] + q[1]
        m.updateState(q, dq, [1, 1, 1, 1], toe, np.zeros(4))
        ref = m.copPlanner_eventbase()
        foot = np.repeat(m.footholdsPlanner()[None], 4, 0)
        x0 = np.array([q[0], dq[0], q[1], dq[1]])
        m.run_NMPC()
        r = oracle.solve_batch(p, x0[None], ref[None], foot[None], Pobs)
        assert conv(m.last_status).tolist() == conv(r["status"][0]).tolist(), (cyc, m.last_status, r["status"])
        assert m.last_status[0] == 0
        np.testing.assert_allclose(xus(4, m.qp_solution_eventbased_), xus(4, r["x_qp"][0]), atol=QP_TOL)   # lambda
        # is not unique with 4 contacts
        np.testing.assert_allclose(m.get_MPCsol().ravel(), r["x"][0][:16], atol=NLP_TOL)
        X = m.get_MPCsol().reshape(4, 4)
        q[0], dq[0], q[1], dq[1] = X[3]
    assert m.gaitDomain_ == 6
