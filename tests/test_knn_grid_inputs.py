"""The inputs of tests/test_knn_grid_small.py, checked on the CPU: every query labelled "through the grid" passes the
gate of knn_select_k as tests/grid_model.py restates it, every query labelled "fall-back" fails it, and outside the
"tiny" and "few finite rows" cases at least three quarters of a case's queries go through the grid.  A check of
the test inputs, not of any kernel."""
import numpy as np
import pytest

import grid_cases
import grid_model
from grid_cases import CASES, KPAIRS


def through(g, q, K, own_row):
    return np.array([grid_model.through_grid(g, x, y, K, own_row) for x, y in q])


def test_header_of_hand_computed_tables():
    """The model itself on tables whose header can be worked out by hand."""
    g = grid_model.header(np.full((300, 2), np.nan))
    assert g == dict(ok=0)
    g = grid_model.header([(0.0, 0.0), (4.0, 4.0)])                       # target 1: h = sqrt(16 / 1)
    assert (g["h"], g["nx"], g["ny"], g["n"]) == (4.0, 2, 2, 2)
    g = grid_model.header([(x, 1.0) for x in np.linspace(0, 100, 300)])    # W H = 0: the floor W / 4096
    assert (g["h"], g["nx"], g["ny"], g["n"]) == (100.0 / 4096.0, 4097, 1, 300)
    g = grid_model.header([(3.5, 3.5)] * 300 + [(np.nan, 0.0)])           # one point: h = sqrt(1e-300 / 150)
    assert (g["nx"], g["ny"], g["n"]) == (1, 1, 300) and 8e-152 < g["h"] < 8.2e-152
    g = grid_model.header([(1e200, 1e200), (-1e200, -1e200)] + [(0.0, 0.0)] * 298)   # W H = inf: h = 1, floor, loop
    assert g["nx"] * g["ny"] <= grid_model.CELLS < (int(2e200 / (g["h"] / 1.25)) + 1) ** 2 and g["nx"] == g["ny"]
    # the gate: cells -63 and nx + 63 are in, -64 and nx + 64 out; fewer rows than K (+ 1) out
    g = grid_model.header([(0.0, 0.0), (4.0, 4.0)])
    assert grid_model.through_grid(g, -62.5 * 4, 0.0, 1) and not grid_model.through_grid(g, -63.5 * 4, 0.0, 1)
    assert grid_model.through_grid(g, 0.0, 65.5 * 4, 1) and not grid_model.through_grid(g, 0.0, 66.5 * 4, 1)
    assert grid_model.through_grid(g, 1.0, 1.0, 2) and not grid_model.through_grid(g, 1.0, 1.0, 3)
    assert grid_model.through_grid(g, 1.0, 1.0, 1, own_row=True) and not grid_model.through_grid(g, 1.0, 1.0, 2, own_row=True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_case_reaches_the_grid_as_labelled(case):
    c = grid_cases.make(case)
    tab, q, lab = c["tab"], c["q"], c["grid"]
    n = len(tab)
    if c.get("quota", True):
        assert lab.mean() >= 0.75, lab.mean()
    g = grid_model.header(tab)
    for K in sorted({k for k, _ in KPAIRS if 0 < k <= n}):
        np.testing.assert_array_equal(through(g, q, K, False), lab, err_msg=f"obstacle pass K {K}")
    if c.get("obs_only"):
        return
    A = min(len(q), n)
    for K in sorted({k for _, k in KPAIRS if 0 < k <= n - 1}):
        for off in grid_cases.offsets(n, A):
            nb = grid_cases.nbr_table(tab, q[:A], off)
            np.testing.assert_array_equal(through(grid_model.header(nb[:, :2]), q[:A], K, True), np.ones(A, bool),
                                          err_msg=f"neighbour pass K {K} off {off}")


@pytest.mark.parametrize("K", [1, 3, 8, 16])
def test_few_finite_rows_labels(K):
    """Fewer finite rows than K (+ 1 with an own row) is the fall-back, K (+ 1) or more the grid."""
    for nbr in (False, True):
        for f in (K - 1, K, K + 1, K + 2):
            tab, q, off, lab = grid_cases.few_finite(np.random.default_rng(100 * K + f), K, f, nbr)
            assert np.isfinite(tab).all(1).sum() == f
            np.testing.assert_array_equal(through(grid_model.header(tab), q, K, nbr), lab, err_msg=f"nbr {nbr} f {f}")
            assert lab.all() == (f >= K + nbr and f > 1) and lab.all() == lab.any()


@pytest.mark.parametrize("Ko,Kn", KPAIRS)
def test_few_finite_rows_inputs_of_every_k_pair(Ko, Kn):
    """The inputs test_grid_few_finite_rows runs, labels against the model; both sides of the gate occur."""
    seen = set()
    for f in grid_cases.few_finite_counts(Ko, Kn):
        q, obs, nbr, off, lab_o, lab_n = grid_cases.few_finite_inputs(Ko, Kn, f)
        if Ko:
            np.testing.assert_array_equal(through(grid_model.header(obs), q, Ko, False), lab_o, err_msg=f"obstacles f {f}")
            seen.add(bool(lab_o.all()))
        if Kn:
            np.testing.assert_array_equal(through(grid_model.header(nbr[:, :2]), q, Kn, True), lab_n, err_msg=f"neighbours f {f}")
            seen.add(bool(lab_n.all()))
            assert np.isnan(nbr[off + 2:off + 4, :2]).all() and (off + 4 <= len(nbr))
    assert seen == {False, True}
