"""CPU tests of the inertia-shift cases (tests/shift_cases.py): the oracle's statistics entry points, and the conditions
every case has to meet before a kernel is compared on it -- all from the oracle alone.  These are conditions, not
measurements: a case that stops meeting them (a changed workload generator, a changed oracle) fails here, on the CPU,
instead of silently comparing nothing on the GPU.
"""
import numpy as np
import pytest

import oracle
import shift_cases as sc

DOCUMENTED = (0, 1, 2, 3, 4)          # OPTIMAL, KKTFAIL, MAXIT, FATAL, ACCEPTABLE (include/srbnmpc.h)


def test_stats_entry_point_leaves_the_results_bit_for_bit():
    """orc_solve_batch and orc_solve_batch_stats (and the SRB-12 pair) return the same bits; without a shift every
    count is zero and the exit rule is one of the residual tests."""
    b, p = sc.lip_batch("n3"), sc.lip_params("n3")
    a = (b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
    r, q = oracle.solve_batch(p, *a, nthreads=4), oracle.solve_batch(p, *a, nthreads=4, stats=True)
    for k in r:
        assert np.array_equal(r[k], q[k]), k
    r0 = oracle.solve_batch(sc.lip_params("n3", Sw=sc.SW_DEFAULT), *a, nthreads=4, stats=True)["stats"]
    assert not r0["failed"].any() and not r0["shift_iters"].any() and not r0["max_tries"].any() and not r0["max_delta"].any()
    assert np.isin(r0["exit"], (oracle.EXIT_RULES.index("converged"), oracle.EXIT_RULES.index("provisional"))).all()
    b = sc.srb12_batch("n10")
    a = (b["x0"][:8], b["xref"][:8], b["foot"][:8], b["contact"][:8], b["obstacles"], b["nbr_state"])
    p = sc.srb12_params("n10")
    r, q = oracle.solve_batch12(p, *a), oracle.solve_batch12(p, *a, stats=True)
    for k in r:
        assert np.array_equal(r[k], q[k]), k


def test_stats_are_consistent():
    """shift_iters <= failed <= 13 shift_iters + (tries exhausted), max_tries <= 14, delta grows tenfold: an agent with
    t failed factorisations in one iteration saw delta >= 1e-10 * 10^(t - 1)."""
    st = sc.lip_case("n11")["r"]["stats"]
    sh = st["failed"] > 0
    assert (st["shift_iters"][sh] >= 1).all() and (st["shift_iters"] <= st["failed"]).all()
    assert (st["max_tries"] <= 14).all() and (st["failed"] <= 14 * st["shift_iters"]).all()
    assert (st["max_delta"][sh] >= 1e-10 * 10.0 ** (st["max_tries"][sh] - 1) * (1 - 1e-12)).all()
    assert (st["max_delta"][~sh] == 0).all() and (st["max_tries"][~sh] == 0).all()
    assert (st["exit"] >= 0).all() and (st["exit"] < len(oracle.EXIT_RULES)).all()


def _floors(name, c, half):
    n = sc.counts(c)
    print(name, n)
    r = c["r"]
    assert np.isin(r["status"], DOCUMENTED).all()
    assert n["shifted_at_default"] == 0, "the batch shifts at the default Sw: the case does not isolate the path"
    assert n["shifted_strict_optimal"] >= 1
    if half:
        assert 2 * n["shifted_strict"] >= n["shifted"], (n["shifted_strict"], n["shifted"])
    # the growth rule is exercised, not only the first shift
    assert n["max_tries"] >= 2
    return n


@pytest.mark.parametrize("name", list(sc.LIP))
def test_lip_case_floors(name):
    c = sc.lip_case(name)
    _floors("LIP " + name, c, half=name not in ("n2", "n3"))
    if name in sc.LIP_EXITS:
        rule, status = sc.LIP_EXITS[name]
        hit = c["shifted"] & c["strict"] & (c["r"]["stats"]["exit"] == oracle.EXIT_RULES.index(rule))
        assert hit.any(), rule
        assert (c["r"]["status"][hit, 1] == status).all()


def test_lip_n20_holds_a_polish_rejected_for_its_matrix():
    """The N = 20 case is also the one whose oracle polish meets a reduced matrix that is not positive definite."""
    assert sc.lip_case("n20")["r"]["stats"]["polish_npd"].any()


@pytest.mark.parametrize("name", list(sc.SRB12))
def test_srb12_case_floors(name):
    _floors("SRB12 " + name, sc.srb12_case(name), half=True)


def test_weights_cases_do_not_shift():
    """Every cost weight (and eps_obs) off its default by a factor that leaves the batch unshifted and every agent
    stable: the GPU comparison holds every agent to the strict rule."""
    for c in (sc.lip_weights_case(), sc.srb12_weights_case()):
        assert not c["r"]["stats"]["failed"].any()
        assert c["strict"].all()
        assert np.isin(c["r"]["status"], DOCUMENTED).all()
    d = oracle.params(10, 2)
    for k, v in sc.LIP_WEIGHTS.items():
        assert getattr(d, k) != v, k
