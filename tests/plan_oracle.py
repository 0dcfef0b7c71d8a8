"""The reference answer for solves against neighbour plans, from the oracle's own pieces.

oracle.solve_batch predicts every neighbour at constant velocity inside orc_solve_agent (oracle/batch.c).
oracle.nlp_solve, though, takes per-grid obstacle positions obs[N][K][2], so the same chain repeated here
per agent -- QP build, QP stage at the warm-start tolerance, selection, NLP stage warm-started from the QP
point -- with the neighbour columns of obs overwritten by rows of a plan table is the oracle's answer for
srb_batch.nbr_plan.  With the constant-velocity table it reproduces oracle.solve_batch bit for bit
(tests/test_nbr_plan.py pins that).
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle

# the shapes of the plan tests: (N, C, K_obs, K_nbr, agents, seed) -- the generic instance, the compiled
# configs[2] instance, the folded-obstacle N = 20 instance with its separate polish kernel, C = 4
SHAPES = [(4, 4, 1, 2, 8, 11), (10, 2, 3, 8, 64, 12), (20, 2, 3, 8, 16, 13), (10, 4, 1, 3, 12, 14)]

_dp = ctypes.POINTER(ctypes.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def cv_table(p, nbr_state):
    """The constant-velocity table: row i, grid k = pos_i + vel_i * (Ts (k + 1)) (nbr_state rows are
    x, y, xdot, ydot), the arithmetic of the oracle's and the kernel's own prediction."""
    nb = np.ascontiguousarray(nbr_state, dtype=np.float64).reshape(-1, 4)
    tt = np.array([p.Ts * (k + 1) for k in range(p.N)])
    return np.ascontiguousarray(nb[:, None, :2] + nb[:, None, 2:] * tt[None, :, None])


def clamped(p, n_obs, n_all):
    """p with K_obs, K_nbr clamped to the tables as the C ABI (and orc_solve_agent) clamp them."""
    q = oracle.OrcParams.from_buffer_copy(p)
    q.K_obs = min(p.K_obs, max(n_obs, 0))
    q.K_nbr = min(p.K_nbr, max(n_all - 1, 0)) if n_all > 0 else 0
    return q


def solve_agent(p, x0, ref, foot, obstacles, nbr_state, table, self_idx, idx=None):
    """orc_solve_agent with the neighbour columns of obs taken from table[idx] (-1 columns keep the
    oracle's no-neighbour row).  p is already clamped.  Returns x_qp, x, obj, status[2], iters[2], idx."""
    nv, neq, mq, _ = oracle.sizes(p)
    Pd, c, A, b, G, h = oracle.build_qp(p, x0, ref, foot)
    tq = p.tol_qp if (p.use_nlp and p.tol_qp > 0.0) else p.tol
    xq = np.zeros(nv); it0 = ctypes.c_int()
    arrs = [np.ascontiguousarray(a) for a in (Pd, c, A, b, G, h)]
    st0 = oracle.lib().orc_qp_solve_init(nv, mq, neq, *[_ptr(a) for a in arrs], p.qp_maxit, ctypes.c_double(tq),
                                         p.qp_init, _ptr(xq), None, ctypes.byref(it0))
    if st0 == 0 and tq > p.tol:
        st0 = 4
    if idx is None:
        idx = oracle.select_idx(p, x0, obstacles, nbr_state, self_idx)
    obs, eps = oracle.select_obstacles(p, x0, obstacles, nbr_state, self_idx)
    obs = np.array(obs, copy=True)
    if table is not None:
        for j in range(p.K_obs, p.K_obs + p.K_nbr):
            if idx[j] >= 0:
                obs[:, j, :] = table[idx[j]]
    x, st1, it1 = oracle.nlp_solve(p, x0, foot, Pd, c, A, b, G, h, obs, eps, xq)
    obj = float(np.sum(0.5 * Pd * x * x + c * x))
    return xq, x, obj, (st0, st1), (it0.value, it1), idx


def solve(p, batch, table, sel=None, agent_offset=0):
    """The batch (workload.make_batch's dict) against the plan table [n_all][N][2] (None: the oracle's own
    constant-velocity rows).  sel [A][Ko + Kn]: rows to use instead of the oracle's snapshot selection."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    A = x0.shape[0]
    ref = np.asarray(batch["ref"]).reshape(A, -1)
    foot = np.asarray(batch["foot"]).reshape(A, -1)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = clamped(p, ob.shape[0], nb.shape[0])
    oracle.lib().orc_qp_solve_init.restype = ctypes.c_int

    def one(a):
        return solve_agent(q, x0[a], ref[a], foot[a], ob, nb, table, agent_offset + a, None if sel is None else sel[a])
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(A)))
    return dict(x_qp=np.array([r[0] for r in res]), x=np.array([r[1] for r in res]),
                obj=np.array([r[2] for r in res]), status=np.array([r[3] for r in res], np.int32),
                iters=np.array([r[4] for r in res], np.int32), sel=np.array([r[5] for r in res], np.int32))


def plans_of(p, x):
    """[A][N][2] CoM positions (x[4k], x[4k + 2]) of decision vectors x [A][nv]."""
    X = np.asarray(x)[:, :4 * p.N].reshape(-1, p.N, 4)
    return np.ascontiguousarray(X[:, :, [0, 2]])


_cache = {}


def reference(shape):
    """For one of SHAPES, computed once and shared (treat as read-only): the batch, the oracle params, the
    constant-velocity oracle answer r0 (oracle.solve_batch), its plans as the table, and the plan-oracle
    answer r1 against that table."""
    if shape not in _cache:
        from srbnmpc import workload
        N, C, Ko, Kn, A, seed = shape
        b = workload.make_batch(A, N, C, seed=seed)
        p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
        r0 = oracle.solve_batch(p, b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nthreads=8)
        table = plans_of(p, r0["x"])
        r1 = solve(p, b, table)
        for r in (r0, r1):
            for v in r.values():
                v.setflags(write=False)
        table.setflags(write=False)
        _cache[shape] = dict(b=b, p=p, r0=r0, table=table, r1=r1)
    return _cache[shape]
