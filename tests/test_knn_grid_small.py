"""The uniform selection grid (srb_grid_build_kernel in csrc/srb_select.hip, the ring search of knn_select_k in
csrc/srb_knn.h) forced onto small tables of hand-designed geometry (tests/grid_cases.py): the option grid_min_rows
= 1 gives every table a grid.  Selection alone (BatchSolver.select_device) against oracle.select_idx, the float64
restatement of the reference's scan -- sqrt distance, lower index on ties, 1000 m / row 0 for obstacles, -1 for
missing neighbours -- compared exactly; then the same context with the grid switched off must give the oracle's
rows too, so a wrong expectation is not blamed on the grid.  tests/grid_model.py says which queries reach the grid
and which fall back to the scan by design (tests/test_knn_grid_inputs.py checks those labels on the CPU)."""
import numpy as np
import pytest

import oracle
import grid_cases
import grid_model
from grid_cases import CASES, KPAIRS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402

N, C = 10, 2
NO_GRID = 2 ** 31 - 1
DEV = torch.device("cuda:0")


def T(v, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=DEV)


def new_solver(Ko, Kn, max_agents=48, grid_min_rows=1):
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), max_agents)
    if grid_min_rows is not None:
        s.set_option("grid_min_rows", grid_min_rows)
    return s


def select(s, q, obs, nbr, off=0, version=0, dev_tabs=None):
    """One srb_select_device call over the tables handed in (None: that pass is left out) into a sel prefilled
    with -7; dev_tabs: device tensors to reuse (a versioned obstacle table is recognised by its address)."""
    ko, kn = s.n_selected(0 if obs is None else len(obs), 0 if nbr is None else len(nbr))
    sel = torch.full((len(q), ko + kn), -7, dtype=torch.int32, device=DEV)
    tob, tnb = dev_tabs if dev_tabs is not None else (None if obs is None else T(obs), None if nbr is None else T(nbr))
    tables = (1 if obs is not None else 0) | (2 if nbr is not None else 0)
    s.select_device(T(grid_cases.x0_of(q)), tob, tnb, sel, tables=tables, agent_offset=off, obstacles_version=version,
                    stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return sel.cpu().numpy()


def want(Ko, Kn, q, obs, nbr, off=0):
    op = oracle.params(N, C, K_obs=Ko if obs is not None else 0, K_nbr=Kn if nbr is not None else 0)
    x0 = grid_cases.x0_of(q)
    ob = obs if obs is not None else np.zeros((0, 2))
    return np.array([oracle.select_idx(op, x0[a], ob, nbr, off + a) for a in range(len(q))], np.int32).reshape(len(q), -1)


def check(s, Ko, Kn, q, obs, nbr, off, msg):
    """Grid run, then the scan on the same context: both the oracle's rows."""
    w = want(Ko, Kn, q, obs, nbr, off)
    np.testing.assert_array_equal(select(s, q, obs, nbr, off), w, err_msg=f"grid: {msg}")
    s.set_option("grid_min_rows", NO_GRID)
    np.testing.assert_array_equal(select(s, q, obs, nbr, off), w, err_msg=f"scan: {msg}")
    s.set_option("grid_min_rows", 1)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_grid_on_small_table(case):
    c = grid_cases.make(case)
    tab, q, lab = c["tab"], c["q"], c["grid"]
    n = len(tab)
    g = grid_model.header(tab)
    ran = 0
    for Ko, Kn in KPAIRS:
        if Ko > n or Kn > n - 1 or (Kn and c.get("obs_only")):
            continue                                   # (tables shorter than K: test_knn_sentinel_and_missing_rows)
        if Ko:                                         # the inputs reach the grid as labelled
            assert [grid_model.through_grid(g, x, y, Ko) for x, y in q] == lab.tolist()
        s = new_solver(Ko, Kn)
        if not Kn:
            check(s, Ko, 0, q, tab, None, 0, f"{case.__name__} K {Ko}+0")
        else:
            A = min(len(q), n)
            for off in grid_cases.offsets(n, A):
                nb = grid_cases.nbr_table(tab, q[:A], off)
                gn = grid_model.header(nb[:, :2])
                assert all(grid_model.through_grid(gn, x, y, Kn, True) for x, y in q[:A])
                check(s, Ko, Kn, q[:A], tab if Ko else None, nb, off, f"{case.__name__} K {Ko}+{Kn} off {off}")
        s.close()
        ran += 1
    assert ran >= {1: 1, 2: 2}.get(n, len(KPAIRS) - (5 if c.get("obs_only") else 0))


@pytest.mark.parametrize("Ko,Kn", KPAIRS)
def test_grid_few_finite_rows(Ko, Kn):
    """Tables with K - 1 .. K + 2 finite rows among NaN ones (never skipped): below K rows (K + 1 with the agent's
    own row, whether that row is finite or NaN) the grid cannot supply K rows and the scan takes over -- row 0
    repeated for obstacles, -1 for missing neighbours -- from K (+ 1) on the grid does."""
    s = new_solver(Ko, Kn, 8)
    for f in grid_cases.few_finite_counts(Ko, Kn):
        q, obs, nbr, off, lab_o, lab_n = grid_cases.few_finite_inputs(Ko, Kn, f)
        if Ko:
            assert [grid_model.through_grid(grid_model.header(obs), x, y, Ko) for x, y in q] == lab_o.tolist()
        if Kn:
            assert [grid_model.through_grid(grid_model.header(nbr[:, :2]), x, y, Kn, True) for x, y in q] == lab_n.tolist()
        check(s, Ko, Kn, q, obs, nbr, off, f"K {Ko}+{Kn} finite rows {f}")
    s.close()


def test_grid_state_across_calls():
    """One context, a sequence of tables: the header goes to ok = 0 on an all-NaN table and back, the grid's
    buffers grow for 5000 rows and are reused for 40, and the threshold option is read at every call."""
    Ko, Kn = 3, 8
    s = new_solver(Ko, Kn)
    rng = np.random.default_rng(77)

    def step(name, tab, q, thresh=1):
        s.set_option("grid_min_rows", thresh)
        n, A = len(tab), len(q)
        off = (n - A) // 2
        nb = grid_cases.nbr_table(tab, q, off)
        if name == "nan":
            nb[:, :2] = np.nan                          # (the agents' own rows too)
        got = select(s, q, tab, nb, off)
        np.testing.assert_array_equal(got, want(Ko, Kn, q, tab, nb, off), err_msg=name)
        return got

    c1, c2 = grid_cases.make(grid_cases.heavy_cell), grid_cases.make(grid_cases.two_clusters)
    step("300 rows", c1["tab"], c1["q"])
    got = step("nan", np.full((300, 2), np.nan), c1["q"])
    assert (got[:, :Ko] == 0).all() and (got[:, Ko:] == -1).all()
    step("300 rows again", c2["tab"], c2["q"])
    big = rng.uniform(-30, 30, (5000, 2))
    qb = np.concatenate([big[:8], rng.uniform(-32, 32, (24, 2))])
    assert all(grid_model.through_grid(grid_model.header(big), x, y, Ko) for x, y in qb)
    step("5000 rows", big, qb)
    c3 = grid_cases.make(CASES[[c.__name__ for c in CASES].index("tiny_40")])
    step("40 rows", c3["tab"], c3["q"])
    step("threshold above the table", c2["tab"], c2["q"], thresh=301)
    step("threshold lowered again", c2["tab"], c2["q"])
    s.close()


def test_versioned_grid_kept_across_scene_calls():
    """grid_min_rows_static = 1, grid_min_rows at its default: only a versioned obstacle table gets a grid.  The
    grid of version 7 is built once, reused, survives calls with scenes on (the scene kernels ignore it), and is
    rebuilt for version 8; version 0 is the scan."""
    Ko, Kn = 3, 8
    s = new_solver(Ko, Kn, grid_min_rows=None)
    s.set_option("grid_min_rows_static", 1)
    c = grid_cases.make(grid_cases.two_clusters)
    tab, q = c["tab"], c["q"]
    A, n = len(q), len(tab)
    assert all(grid_model.through_grid(grid_model.header(tab), x, y, Ko) for x, y in q)
    tob = T(tab)

    def static(ver, table):
        tob.copy_(T(table))
        got = select(s, q, table, None, version=ver, dev_tabs=(tob, None))
        np.testing.assert_array_equal(got, want(Ko, 0, q, table, None), err_msg=f"version {ver}")

    static(7, tab)
    static(7, tab)
    # scenes: 4 teams of 6 agents, 75 obstacle rows each; every agent selects within its own scene (global rows)
    sa, so = A // 4, n // 4
    assert sa * 4 == A and so * 4 == n
    s.set_scenes(sa, so)
    nb = grid_cases.nbr_table(tab[:A], q, 0)
    ko, kn = s.n_selected(n, A)
    sel = torch.full((A, ko + kn), -7, dtype=torch.int32, device=DEV)
    s.select_device(T(grid_cases.x0_of(q)), tob, T(nb), sel, tables=3, obstacles_version=7,
                    stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    got = sel.cpu().numpy()
    op = oracle.params(N, C, K_obs=ko, K_nbr=kn)
    x0 = grid_cases.x0_of(q)
    for a in range(A):
        sc = a // sa
        w = oracle.select_idx(op, x0[a], tab[sc * so:(sc + 1) * so], nb[sc * sa:(sc + 1) * sa], a - sc * sa)
        w = np.concatenate([w[:ko] + sc * so, np.where(w[ko:] >= 0, w[ko:] + sc * sa, -1)])
        np.testing.assert_array_equal(got[a], w, err_msg=f"scene {sc} agent {a}")
    s.set_scenes(0, 0)
    static(7, tab)                                        # the kept grid (no rebuild: same version, address, size)
    static(8, tab[::-1].copy())
    static(0, tab[::-1].copy())
    s.close()


def test_solve_with_forced_grid_equals_default_threshold():
    """BatchSolver.solve on the two-clusters tables with the grid forced and with the default threshold (the scan):
    sel, status and x bit-identical, sel the oracle's."""
    Ko, Kn, A = 3, 8, 32
    c = grid_cases.make(grid_cases.two_clusters)
    b = workload.make_batch(A, N, C, seed=14)
    ob = c["tab"] + (4.0, 6.0)                           # the first cluster beside the arena, not on the agents
    n = len(ob)
    off = (n - A) // 2
    nb = np.zeros((n, 4)); nb[:, :2] = c["tab"][::-1] + (4.0, -6.0)
    nb[off:off + A] = b["nbr_state"]
    gq = [(x, y) for x, y in b["x0"][:, [0, 2]]]
    assert all(grid_model.through_grid(grid_model.header(ob), x, y, Ko) for x, y in gq)
    assert all(grid_model.through_grid(grid_model.header(nb[:, :2]), x, y, Kn, True) for x, y in gq)
    outs = []
    for thresh in (1, None):
        s = new_solver(Ko, Kn, A, grid_min_rows=thresh)
        outs.append(s.solve(b["x0"], b["ref"], b["foot"], ob, nb, agent_offset=off))
        s.close()
    for k in ("sel", "status", "x"):
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
    op = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    w = np.array([oracle.select_idx(op, b["x0"][a], ob, nb, off + a) for a in range(A)], np.int32)
    np.testing.assert_array_equal(outs[0]["sel"], w)
