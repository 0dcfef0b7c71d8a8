"""Reference answers for SRB-12 solves against neighbour plans (srb12_plans), from the oracle's own pieces.

orc12_solve_agent predicts every neighbour itself, at constant velocity from the snapshot row, so no oracle answers
an arbitrary plan table.  Two answers exist all the same:

  linear tables   T[i][k] = p_i + w_i * (Ts * (k + 1)) with w_i drawn independently of the snapshot velocity v_i.
                  The selection reads positions only and the query x0 is unchanged, so the device's answer for
                  (nbr_state (p_i, v_i), table T) must equal oracle.solve_batch12 for the snapshot (p_i, w_i):
                  `reference(shape)` holds both oracle runs.
  curved tables   `rows` builds the per-grid rows obs[N][K][2] of one agent from the selection plus the table, and
                  `certificate` runs kkt.certify on test_srb12._problem with them: an independent KKT certificate
                  of the point, whatever the table.

`shift` restates dist.shift_plans in numpy (the rollout's table of the next cycle).
"""
import numpy as np

import oracle
from kkt import certify
from srbnmpc import workload
from test_srb12 import _problem

# (N, K_obs, K_nbr, agents, gait, workload.make_batch12 seed)
SHAPES12 = [(10, 3, 8, 16, "trot", 41), (10, 3, 8, 16, "stand", 42), (4, 1, 2, 8, "trot", 45),
            (20, 3, 8, 8, "trot", 44), (6, 2, 3, 12, "stand", 45)]
SHIFT_GRIDS = 4                                             # one gait domain a cycle


def lip_params(p):
    """The LIP-mode oracle parameters with p's selection and prediction constants (oracle.select_idx /
    select_obstacles are the LIP mode's)."""
    return oracle.params(p.N, 2, K_obs=p.K_obs, K_nbr=p.K_nbr, Ts=p.Ts, eps_obs=p.eps_obs, eps_nbr=p.eps_nbr)


def lip_x0(x0):
    """[x, xdot, y, ydot] of a 12-state x0: the row the selection reads."""
    return np.array([x0[0], x0[6], x0[1], x0[7]])


def linear_table(p, pos, w):
    """T[i][k] = pos_i + w_i * (Ts * (k + 1)), the operation order of the oracle's and the kernel's own
    constant-velocity prediction."""
    tt = np.array([p.Ts * (k + 1) for k in range(p.N)])
    pos, w = np.asarray(pos, np.float64), np.asarray(w, np.float64)
    return np.ascontiguousarray(pos[:, None, :] + w[:, None, :] * tt[None, :, None])


def cv_table(p, nbr_state):
    """The constant-velocity table of a snapshot [n][4] (x, y, xdot, ydot)."""
    nb = np.asarray(nbr_state, np.float64).reshape(-1, 4)
    return linear_table(p, nb[:, :2], nb[:, 2:])


def plans_of(N, x):
    """[A][N][2]: (X[12k], X[12k+1]) of decision vectors x [A][24N+1] -- srb12_plans.plan."""
    X = np.asarray(x)[:, :12 * N].reshape(-1, N, 12)
    return np.ascontiguousarray(X[:, :, :2])


def shift(plan, grids=SHIFT_GRIDS):
    """dist.shift_plans in numpy: table[a][k] = plan[a][k + grids] for k < N - grids, past the horizon
    last + m (last - previous), m = k + grids - N + 1."""
    plan = np.asarray(plan, np.float64)
    n, N, _ = plan.shape
    if grids < 0 or N < 2:
        raise ValueError("shift: grids >= 0 and N >= 2")
    out = np.empty_like(plan)
    keep = max(N - grids, 0)
    out[:, :keep] = plan[:, grids:]
    last, diff = plan[:, N - 1], plan[:, N - 1] - plan[:, N - 2]
    for k in range(keep, N):
        out[:, k] = last + float(k + grids - N + 1) * diff
    return out


def select(p, b, a, self_idx=None):
    """The snapshot selection of agent a of batch b (K_obs static rows, then K_nbr neighbour rows, -1: none)."""
    return oracle.select_idx(lip_params(p), lip_x0(b["x0"][a]), b["obstacles"], b["nbr_state"],
                             int(a if self_idx is None else self_idx))


def rows(p, b, a, table, sel=None, self_idx=None):
    """obs [N][K][2], eps [K] of agent a: the static columns from the obstacle table, the neighbour columns from
    table[sel[j]] (None: the constant-velocity prediction of the snapshot), a -1 column the no-neighbour row
    x0 + 1000 m.  sel: the rows to use instead of the snapshot selection."""
    if sel is None:
        sel = select(p, b, a, self_idx)
    Ko, N = p.K_obs, p.N
    Kn = len(sel) - Ko                                      # (the device clamps its columns to the rows that exist)
    x0 = b["x0"][a]
    if table is None:
        table = cv_table(p, b["nbr_state"])
    obs = np.zeros((N, Ko + Kn, 2))
    for j in range(Ko + Kn):
        i = int(sel[j])
        if i < 0:
            obs[:, j] = (x0[0] + 1000.0, x0[1])
        elif j < Ko:
            obs[:, j] = np.asarray(b["obstacles"]).reshape(-1, 2)[i]
        else:
            obs[:, j] = table[i]
    eps = np.array([p.eps_obs] * Ko + [p.eps_nbr] * Kn)
    return obs, eps


def certificate(p, b, a, obs, eps, x):
    """kkt.certify of the point x on agent a's problem with the rows obs: dict(eq, prim, stat_rel, ..)."""
    Pd, c, Aeq, beq, gJ, hh = _problem(p, b["x0"][a], b["xref"][a], b["foot"][a], b["contact"][a], obs, eps)
    return certify(Pd, c, Aeq, beq, gJ, hh, x)


_cache = {}


def reference(shape):
    """For one of SHAPES12, computed once and shared (read-only): the batch b, the oracle params p, the velocities w
    and the linear table, the constant-velocity oracle answer r_cv (snapshot (p_i, v_i)) and the oracle answer
    r_lin for the snapshot (p_i, w_i), which is the answer for (nbr_state, table)."""
    if shape not in _cache:
        N, Ko, Kn, A, gait, seed = shape
        b = workload.make_batch12(A, N, gait, seed=seed)
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        w = np.random.default_rng(seed + 1000).uniform(-0.6, 0.6, (A, 2))
        nbr_lin = np.ascontiguousarray(np.concatenate([b["nbr_state"][:, :2], w], 1))
        table = linear_table(p, b["nbr_state"][:, :2], w)
        args = (b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"])
        r_cv = oracle.solve_batch12(p, *args, b["nbr_state"])
        r_lin = oracle.solve_batch12(p, *args, nbr_lin)
        for r in (r_cv, r_lin):
            for v in r.values():
                v.setflags(write=False)
        for v in (w, nbr_lin, table):
            v.setflags(write=False)
        _cache[shape] = dict(b=b, p=p, w=w, nbr_lin=nbr_lin, table=table, r_cv=r_cv, r_lin=r_lin)
    return _cache[shape]
