"""Hand-designed geometries for the selection grid on small tables (tests/test_knn_grid_small.py runs them on the
GPU, tests/test_knn_grid_inputs.py checks on the CPU that they reach the code they are meant to reach).

A case is a function of a seeded rng returning dict(tab [n][2], q [A][2], grid [A] bool): the table's positions,
the query points, and for each query whether it is meant to go through the grid when the table is the obstacle
table (tables & 1: free query points).  In the neighbour pass (tables & 2) the queries overwrite rows
off .. off + A of the table, so every query lies inside the grid's bounds and is meant to go through it.
Optional keys: obs_only (no neighbour pass), quota (False: the three-quarters rule does not apply)."""
import numpy as np

import grid_model

N_TAB = 300
KPAIRS = [(1, 0), (3, 0), (16, 0), (0, 1), (0, 8), (0, 16), (3, 8), (16, 16)]


def _case(tab, q, grid, **kw):
    tab, q = np.asarray(tab, np.float64).reshape(-1, 2), np.asarray(q, np.float64).reshape(-1, 2)
    grid = np.asarray(grid, bool)
    assert len(q) == len(grid) <= 48
    return dict(tab=tab, q=q, grid=grid, **kw)


def _swap(c):
    """The same case with x and y exchanged."""
    return dict(c, tab=c["tab"][:, ::-1].copy(), q=c["q"][:, ::-1].copy())


def collinear_x(rng):
    """y constant, span 100 m: W*H == 0, h from the /4096 floor (0.0244 m), a 4097 x 1 grid.  5 m off the line
    and 3 m past an end are more than 64 cells (1.56 m) away: fall-back."""
    x = rng.uniform(0, 100, N_TAB); x[:2] = (0.0, 100.0)
    tab = np.stack([x, np.full(N_TAB, -1.75)], 1)
    on = np.concatenate([x[2:10], rng.uniform(0, 100, 8)])
    q = [(v, -1.75) for v in on]
    q += [(v, -1.75 + s * 0.3) for v, s in zip(rng.uniform(0, 100, 8), (1, -1) * 4)]
    q += [(v, -1.75 + s * 5.0) for v, s in zip(rng.uniform(0, 100, 4), (1, -1) * 2)]
    q += [(-1.0, -1.75), (101.0, -1.75), (-3.0, -1.75), (103.0, -1.75)]
    return _case(tab, q, [True] * 16 + [True] * 8 + [False] * 4 + [True, True, False, False])


def collinear_y(rng):
    """x = 7.25, y on a quarter-metre lattice over 100 m (duplicates, exact ties): a 1 x 4097 grid."""
    y = rng.integers(0, 401, N_TAB) / 4.0; y[:2] = (0.0, 100.0)
    tab = np.stack([np.full(N_TAB, 7.25), y], 1)
    on = np.concatenate([y[2:10], rng.integers(0, 401, 4) / 4.0 + 0.125, rng.uniform(0, 100, 4)])
    q = [(7.25, v) for v in on]
    q += [(7.25 + s * 0.3, v) for v, s in zip(rng.integers(0, 401, 8) / 4.0, (1, -1) * 4)]
    q += [(7.25 + s * 5.0, v) for v, s in zip(rng.uniform(0, 100, 4), (1, -1) * 2)]
    q += [(7.25, -1.0), (7.25, 101.0), (7.25, -3.0), (7.25, 103.0)]
    return _case(tab, q, [True] * 16 + [True] * 8 + [False] * 4 + [True, True, False, False])


def gap_line_x(rng):
    """150 rows in [0, 1], 150 in [99, 100] on the line y = 2: from the middle of the gap the ring loop runs to
    r0 ~ 2000 over one cell row thousands of cells wide (gap_line_y: dozens of 64-row batches)."""
    x = np.concatenate([rng.uniform(0, 1, 150), rng.uniform(99, 100, 150)]); x[0] = 0.0; x[-1] = 100.0
    tab = np.stack([x, np.full(N_TAB, 2.0)], 1)
    qx = [50.0, 49.5, 50.5, 30.0, 70.0, 1.5, 98.5, 0.5, 99.5, 0.25, 99.75, -0.5, 100.5, -1.5, 101.5, 5.0]
    q = [(v, 2.0) for v in qx] + [(50.0, 2.2), (50.0, 1.0), (0.5, 2.9), (99.5, 1.1)]
    return _case(tab, q, [True] * 20)


def gap_line_y(rng):
    return _swap(gap_line_x(rng))


def thin_strip(rng):
    """x in [0, 1000], y in [0, 1e-9]: W*H tiny but not 0, h = 1000 / 4096 from the floor, a 4097 x 1 grid."""
    x = rng.uniform(0, 1000, N_TAB); x[:2] = (0.0, 1000.0)
    y = rng.uniform(0, 1e-9, N_TAB); y[2:4] = (0.0, 1e-9)
    tab = np.stack([x, y], 1)
    q = [(v, 0.0) for v in x[4:12]] + [(v, 5e-10) for v in rng.uniform(0, 1000, 8)]
    q += [(v, s) for v, s in zip(rng.uniform(0, 1000, 8), (1.0, -1.0) * 4)]
    q += [(1005.0, 0.0), (-5.0, 0.0), (1050.0, 0.0), (-50.0, 0.0)]
    return _case(tab, q, [True] * 24 + [True, True, False, False])


def coincident(rng):
    """Every row at (3.5, 3.5): W = H = 0, h ~ 1e-152, one cell, index order among equal distances.  A query
    0.1 m away is 1e150 cells away: fall-back."""
    tab = np.full((N_TAB, 2), 3.5)
    q = [(3.5, 3.5)] * 6 + [(3.6, 3.5), (3.5, 3.4)]
    return _case(tab, q, [True] * 6 + [False] * 2)


def heavy_cell(rng):
    """Rows 50 .. 249 at one point: more than 64 candidates in one cell, several trips of the candidate loop,
    and the K lowest indices whatever order the atomic scatter used."""
    tab = rng.uniform(-8, 8, (N_TAB, 2)); tab[50:250] = (1.25, -2.5)
    ang = np.arange(8) * (np.pi / 4)
    q = [(1.25, -2.5)] * 4 + [(1.25 + 0.25 * np.cos(a), -2.5 + 0.25 * np.sin(a)) for a in ang]
    q += [(0.0, 0.0), (0.0, 0.0)] + [tuple(v) for v in rng.uniform(-8, 8, (10, 2))]
    return _case(tab, q, [True] * 24)


def cluster_outlier(rng):
    """normal(0, 0.5) with one row at (4000, -3000): cells of some 280 m, nearly every row in one cell, and
    queries with no obstacle within 1000 m (row 0 repeated) on the grid path."""
    tab = rng.normal(0, 0.5, (N_TAB, 2)); tab[7] = (4000.0, -3000.0)
    q = [tuple(v) for v in rng.normal(0, 0.5, (10, 2))] + [tuple(tab[3]), tuple(tab[250])]
    q += [(2000.0, -1500.0), (2000.5, -1499.0), (4000.0, -3000.0), (4000.5, -3000.5), (3999.0, -2999.0), (3200.0, -2400.0)]
    return _case(tab, q, [True] * 18)


def two_clusters(rng):
    """normal(0, 0.3) at (0, 0) and (200, 50): empty cell rows between full ones, rings past 4."""
    tab = np.concatenate([rng.normal(0, 0.3, (150, 2)), rng.normal(0, 0.3, (150, 2)) + (200.0, 50.0)])
    q = [tuple(v) for v in rng.normal(0, 0.3, (8, 2))] + [tuple(v + (200.0, 50.0)) for v in rng.normal(0, 0.3, (8, 2))]
    q += [(100.0, 25.0), (100.0, 0.0), (60.0, 40.0), (150.0, 10.0), (-30.0, -30.0), (260.0, 90.0), (0.0, 50.0), (200.0, 0.0)]
    return _case(tab, q, [True] * 24)


def lattice(rng):
    """A quarter-metre lattice in [-6, 6]^2 (many duplicates) queried on a 0.75 m lattice over [-7, 7]^2: exact
    ties across cell borders; rows 60 .. 67 hold sqrt-rounding ties of queries 0 .. 3 (the farther d^2 at the
    lower index)."""
    from test_oracle import sqrt_tie_pair
    tab = rng.integers(-24, 25, (N_TAB, 2)) / 4.0
    g = np.arange(-7.0, 7.01, 0.75)
    pts = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    q = pts[rng.choice(len(pts), 44, replace=False)]
    q[4:8] = [(-7.0, -7.0), (6.5, 6.5), (-7.0, 6.5), (0.5, 0.5)]
    # (a pair 0.3 .. 0.4 m away is among the nearest rows; its y near 0, where the doubles are dense enough
    # for two d^2 to share a sqrt)
    q[0:4] = [(-4.0, -0.25), (-0.25, -0.25), (2.0, -0.25), (5.0, -0.25)]
    for a in range(4):
        near, far = sqrt_tie_pair(q[a, 0], q[a, 1], rng, lo=0.2, hi=0.3)
        tab[60 + 2 * a], tab[61 + 2 * a] = far, near
    return _case(tab, q, [True] * 44)


def boundary(rng):
    """Queries on and a hair outside the grid's bounds: fx == nx, fx == -1, the clamp of grid_cell."""
    tab = rng.uniform(0, 10, (N_TAB, 2)); tab[0] = (0.0, 0.0); tab[1] = (10.0, 10.0)
    q = [(0.0, 0.0), (10.0, 10.0), (0.0, 10.0), (10.0, 0.0), (10.0000001, 10.0), (-1e-9, 5.0), (10.0, 5.0), (5.0, 10.0),
         (0.0, 5.0), (5.0, 0.0), (5.0, -1e-9), (5.0, 10.0000001)] + [tuple(v) for v in rng.uniform(0, 10, (8, 2))]
    return _case(tab, q, [True] * 20)


def outside(rng):
    """Queries c = 10, 63, 64, 65 cells beyond the first and the last cell on every side, placed by the model's
    h at mid-cell: the gate -64 < fx < nx + 64 admits cells -63 and nx + 63 and refuses -64 and nx + 64."""
    tab = rng.uniform(0, 10, (N_TAB, 2)); tab[0] = (0.0, 0.0); tab[1] = (10.0, 10.0)
    g = grid_model.header(tab)
    h, nx, ny = g["h"], g["nx"], g["ny"]
    q, lab = [], []
    for c in (10, 63, 64, 65):
        q += [(-(c - 0.5) * h, 5.0), (5.0, -(c - 0.5) * h)]; lab += [c <= 63] * 2              # cells -c
        q += [((nx - 0.5 + c) * h, 5.0), (5.0, (ny - 0.5 + c) * h)]; lab += [c <= 64] * 2       # cells nx - 1 + c
    q += [tuple(v) for v in rng.uniform(-3, 13, (14, 2))]
    return _case(tab, q, lab + [True] * 14, obs_only=True)


def _tiny(n):
    def case(rng):
        """n = 1 (target = 1, W = H = 0: only a query on the row itself is in the one cell), 2, 17, 40."""
        tab = rng.uniform(0, 4, (40, 2))[:n]; tab[0] = (0.0, 0.0)
        if n > 1:
            tab[1] = (4.0, 4.0)
        q = [(0.0, 0.0), (1.0, 3.0), (2.5, 0.5), (3.0, 3.0), (-0.5, -0.5), (1000.0, 1000.0)]
        return _case(tab, q, [True] + [n > 1] * 4 + [False], quota=False)
    case.__name__ = f"tiny_{n}"
    return case


def _huge(outliers):
    def case(rng):
        """Uniform in [-1e6, 1e6]^2: the 1000 m rule everywhere.  With rows 3, 4 at +-1e200 W*H overflows: h = 1,
        then the /4096 floor and the 1.25 loop."""
        tab = rng.uniform(-1e6, 1e6, (N_TAB, 2))
        if outliers:
            tab[3] = (1e200, 1e200); tab[4] = (-1e200, -1e200)
        q = [(0.0, 0.0)] + [tuple(tab[i]) for i in (0, 9, 150, 299)] + [tuple(tab[20] + (300.0, -400.0)), tuple(tab[21] + (800.0, 700.0))]
        q += [tuple(v) for v in rng.uniform(-1e6, 1e6, (9, 2))]
        return _case(tab, q, [True] * 16)
    case.__name__ = "huge_1e200" if outliers else "huge"
    return case


CASES = [collinear_x, collinear_y, gap_line_x, gap_line_y, thin_strip, coincident, heavy_cell, cluster_outlier,
         two_clusters, lattice, boundary, outside, _tiny(1), _tiny(2), _tiny(17), _tiny(40), _huge(False), _huge(True)]


def make(case):
    """The case's inputs, from a generator seeded by its name (the same on every call)."""
    return case(np.random.default_rng(list(case.__name__.encode())))


def offsets(n, A):
    """agent_offset values of the neighbour pass: the table's start, its middle, its end."""
    return sorted({0, (n - A) // 2, n - A})


def nbr_table(tab, q, off):
    """The neighbour snapshot [n][4] of a case: rows off .. off + A are the agents (the query points), velocities
    arbitrary (the selection reads the positions alone)."""
    nb = np.zeros((len(tab), 4))
    nb[:, :2] = tab
    nb[off:off + len(q), :2] = q
    nb[:, 2:] = 0.125
    return nb


def x0_of(q):
    """Agent states [A][4] = (x, xdot, y, ydot) at the query points."""
    x0 = np.zeros((len(q), 4))
    x0[:, 0], x0[:, 2] = q[:, 0], q[:, 1]
    return x0


def few_finite(rng, K, f, nbr):
    """A table of N_TAB rows with f finite ones, the first two of them at (-1, -1) and (11, 11) and the others
    uniform in [0, 10]^2, so that from two finite rows on every query lies inside the grid's bounds (one finite row
    alone is a grid of one cell some 1e-150 m wide, which no other point is in).  Obstacle form: the finite rows at
    random indices, 8 free queries.  Neighbour form (off = 140, 4 agents): the rows of agents 0, 1 -- the two
    corners -- hold their positions, those of agents 2, 3 stay NaN (an agent whose own row is missing), the other
    finite rows are random.  Returns (table positions, q, off, through-the-grid label per query): the grid needs K
    finite rows, in the neighbour pass K + 1 -- the own-row allowance, claimed whether or not the own row is
    finite."""
    tab = np.full((N_TAB, 2), np.nan)
    corners = np.array([(-1.0, -1.0), (11.0, 11.0)])
    if not nbr:
        rows = rng.choice(N_TAB, f, replace=False)
        tab[rows] = np.concatenate([corners, rng.uniform(0, 10, (max(f - 2, 0), 2))])[:f]
        return tab, rng.uniform(0, 10, (8, 2)), 0, np.full(8, f >= K and f > 1)
    off, q = 140, np.concatenate([corners, rng.uniform(0, 10, (2, 2))])
    own = min(f, 2)
    tab[off:off + own] = q[:own]
    rest = rng.choice(np.setdiff1d(np.arange(N_TAB), np.arange(off, off + 4)), f - own, replace=False)
    tab[rest] = rng.uniform(0, 10, (f - own, 2))
    return tab, q, off, np.full(4, f >= K + 1 and f > 1)


def few_finite_counts(Ko, Kn):
    """Finite-row counts of the few-finite-rows case for a K pair: K - 1 .. K + 2 of either side."""
    return sorted({k + d for k in (Ko, Kn) if k for d in (-1, 0, 1, 2)})


def few_finite_inputs(Ko, Kn, f):
    """The few-finite-rows inputs of a K pair: (q, obstacles or None, neighbour snapshot [n][4] or None, off,
    labels of the obstacle pass or None, labels of the neighbour pass or None).  With both tables the queries are
    the neighbour form's agents."""
    rng = np.random.default_rng(1000 * Ko + 10 * Kn + f)
    q = obs = nbr = lab_o = lab_n = None
    off = 0
    if Kn:
        tn, q, off, lab_n = few_finite(rng, Kn, f, True)
        nbr = np.concatenate([tn, np.full((len(tn), 2), 0.25)], 1)
    if Ko:
        obs, qo, _, lab_o = few_finite(rng, Ko, f, False)
        q = qo if q is None else q
        lab_o = lab_o[:len(q)]
    return q, obs, nbr, off, lab_o, lab_n
