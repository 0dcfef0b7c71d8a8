"""The reference answers for agent sizes (srb_agent_sizes), from the oracle's own pieces and numpy.

solve() is sizes_oracle.solve_agent's chain -- QP build, QP stage at the warm-start tolerance, selection, NLP stage
warm-started from the QP point -- with the levels oracle.nlp_solve takes per column overwritten by the two expressions
of the header, rad then pad: eps[K_obs + j] = s * s, s = rad[g] + rad[idx[K_obs + j]] for every neighbour column with
a row (a -1 column keeps eps_nbr), and eps[:K_obs] = t * t, t = sqrt(eps[:K_obs]) + pad[g], g the agent's own table
row.  Without a table it is oracle.solve_batch bit for bit (tests/test_agent_sizes.py pins that).

nbr_clear_keys() / nbr_clear_select() restate srb_knn_nbr_clear_kernel: the key dist_i - rad[i] with dist_i the
snapshot distance, or with a plan table the sqrt of the horizon-aware selection's minimum over the N + 1 pairs; a
stable sort on (key, index), the own row left out, NaN keys never selected, -1 where no row is left.  numpy neither
fuses a multiply-add nor reorders a sum and its sqrt rounds correctly, so the comparison with the device is index for
index.  Metrics is srb_sim_metrics_agents_kernel, bit for bit.

closed_loop() is the oracle-only closed loop with agent sizes on sim_oracle's advance and next_state.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import moving_oracle
import oracle
import plan_oracle
import sim_oracle
import sizes_oracle
from srbnmpc import workload

RUNS = moving_oracle.RUNS


def levels(p, eps, idx, g, rad=None, pad=None):
    """The levels of the K columns after the agent tables, rad then pad (eps: after the obs_eps gather)."""
    eps = np.array(eps, dtype=np.float64, copy=True)
    if rad is not None:
        rad = np.asarray(rad, dtype=np.float64)
        for j in range(p.K_obs, p.K_obs + p.K_nbr):
            if idx[j] >= 0:
                s = rad[g] + rad[idx[j]]
                eps[j] = s * s
    if pad is not None and p.K_obs > 0:
        t = np.sqrt(eps[:p.K_obs]) + np.asarray(pad, dtype=np.float64)[g]
        eps[:p.K_obs] = t * t
    return eps


def solve_agent(p, x0, ref, foot, obstacles, obs_eps, vel, nbr_state, table, self_idx, rad, pad, idx=None):
    """sizes_oracle.solve_agent (obs_eps None: eps_obs for every static column) with the levels rewritten by
    levels().  p is already clamped.  Returns x_qp, x, obj, status[2], iters[2], idx."""
    nv, neq, mq, _ = oracle.sizes(p)
    Pd, c, A, b, G, h = oracle.build_qp(p, x0, ref, foot)
    tq = p.tol_qp if (p.use_nlp and p.tol_qp > 0.0) else p.tol
    xq = np.zeros(nv); it0 = ctypes.c_int()
    arrs = [np.ascontiguousarray(a) for a in (Pd, c, A, b, G, h)]
    st0 = oracle.lib().orc_qp_solve_init(nv, mq, neq, *[plan_oracle._ptr(a) for a in arrs], p.qp_maxit, ctypes.c_double(tq),
                                         p.qp_init, plan_oracle._ptr(xq), None, ctypes.byref(it0))
    if st0 == 0 and tq > p.tol:
        st0 = 4
    given = idx is not None
    if not given:
        idx = oracle.select_idx(p, x0, obstacles, nbr_state, self_idx)
    obs, eps = oracle.select_obstacles(p, x0, obstacles, nbr_state, self_idx)
    obs, eps = np.array(obs, copy=True), np.array(eps, copy=True)
    if p.K_obs > 0:
        rows = np.asarray(idx[:p.K_obs])
        if given or vel is not None:
            v = np.zeros_like(np.asarray(obstacles, dtype=np.float64).reshape(-1, 2)) if vel is None else vel
            obs[:, :p.K_obs, :] = moving_oracle.moved_rows(p, obstacles, v, rows)
        if obs_eps is not None:
            eps[:p.K_obs] = np.asarray(obs_eps, dtype=np.float64)[rows]
    if table is None and given and p.K_nbr > 0:
        table = plan_oracle.cv_table(p, nbr_state)          # the oracle's own rows, bit for bit, for the given idx
    if table is not None:
        for j in range(p.K_obs, p.K_obs + p.K_nbr):
            if idx[j] >= 0:
                obs[:, j, :] = table[idx[j]]
    eps = levels(p, eps, idx, self_idx, rad, pad)
    x, st1, it1 = oracle.nlp_solve(p, x0, foot, Pd, c, A, b, G, h, obs, eps, xq)
    obj = float(np.sum(0.5 * Pd * x * x + c * x))
    return xq, x, obj, (st0, st1), (it0.value, it1), np.asarray(idx, np.int32)


def solve(p, batch, rad=None, pad=None, obs_eps=None, vel=None, sel=None, table=None, agent_offset=0):
    """The batch (workload.make_batch's dict) with the agent tables rad / pad [n_all] (None: absent), obstacles of
    levels obs_eps (None: eps_obs) moving at vel (None: static), neighbour rows from table (None: constant velocity)."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    A = x0.shape[0]
    ref = np.asarray(batch["ref"]).reshape(A, -1)
    foot = np.asarray(batch["foot"]).reshape(A, -1)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = plan_oracle.clamped(p, ob.shape[0], nb.shape[0])
    oracle.lib().orc_qp_solve_init.restype = ctypes.c_int

    def one(a):
        return solve_agent(q, x0[a], ref[a], foot[a], ob, obs_eps, vel, nb, table, agent_offset + a, rad, pad,
                           None if sel is None else sel[a])
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(A)))
    return dict(x_qp=np.array([r[0] for r in res]), x=np.array([r[1] for r in res]),
                obj=np.array([r[2] for r in res]), status=np.array([r[3] for r in res], np.int32),
                iters=np.array([r[4] for r in res], np.int32), sel=np.array([r[5] for r in res], np.int32))


# ---------------------------------------------------------------------------- neighbour clearance selection
def nbr_clear_keys(x0, nbr, rad, plan=None, lo=0):
    """[A][n_all]: dist_i - rad[i] for agents lo .. lo + A of the table; dist_i the snapshot distance
    sqrt(dx*dx + dy*dy), or with plan [n_all][N][2] the sqrt of the minimum over the snapshot pair and the N plan
    pairs (own plan row lo + a).  NaN where the row, a plan point or the radius is NaN."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 4)
    nbr = np.asarray(nbr, dtype=np.float64).reshape(-1, 4)
    rad = np.asarray(rad, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = x0[:, 0, None] - nbr[None, :, 0], x0[:, 2, None] - nbr[None, :, 1]
        d2 = dx * dx + dy * dy
        if plan is not None:
            plan = np.asarray(plan, dtype=np.float64)
            own = plan[lo:lo + x0.shape[0]]
            ex, ey = own[:, None, :, 0] - plan[None, :, :, 0], own[:, None, :, 1] - plan[None, :, :, 1]
            d2 = np.min(np.concatenate([d2[:, :, None], ex * ex + ey * ey], 2), 2)      # np.min propagates NaN
        return np.sqrt(d2) - rad[None]


def by_key(key, K, lo=0, base=0):
    """[A][K]: rows in (key, index) order, the own row (lo + a) left out, NaN keys never, -1 where no row is left."""
    A, n = key.shape
    out = np.full((A, K), -1, np.int32)
    for a in range(A):
        order = [i for i in np.lexsort((np.arange(n), key[a])) if i != lo + a and not np.isnan(key[a, i])]
        order = order[:K]
        out[a, :len(order)] = np.asarray(order, np.int32) + base
    return out


def nbr_clear_select(x0, nbr, rad, K, plan=None, lo=0, scene_agents=0):
    """The neighbour columns of srb_knn_nbr_clear_kernel for agents lo .. of the table, K clamped to the other rows
    as the C ABI clamps it; with scenes, of its scene form (global indices)."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 4)
    nbr = np.asarray(nbr, dtype=np.float64).reshape(-1, 4)
    rad = np.asarray(rad, dtype=np.float64)
    if scene_agents <= 0:
        return by_key(nbr_clear_keys(x0, nbr, rad, plan, lo), min(K, max(nbr.shape[0] - 1, 0)), lo)
    rows = []
    for a in range(x0.shape[0]):
        n0 = ((lo + a) // scene_agents) * scene_agents
        sl = slice(n0, n0 + scene_agents)
        key = nbr_clear_keys(x0[a:a + 1], nbr[sl], rad[sl], None if plan is None else np.asarray(plan)[sl], lo + a - n0)
        rows.append(by_key(key, min(K, scene_agents - 1), lo + a - n0, n0)[0])
    return np.array(rows, np.int32)


def full_sel(p, batch, nbr_cols, static_cols=None):
    """[A][Ko + Kn]: nbr_cols beside static_cols (None: the oracle's own static columns)."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = plan_oracle.clamped(p, ob.shape[0], nb.shape[0])
    if static_cols is None:
        static_cols = np.array([oracle.select_idx(q, x0[a], ob, nb, a) for a in range(x0.shape[0])], np.int32)[:, :q.K_obs]
    return np.concatenate([np.asarray(static_cols, np.int32), np.asarray(nbr_cols, np.int32)], 1)


# ---------------------------------------------------------------------------- metrics
def body_clearance(px, py, table, body, skip):
    """min over i != skip of (sqrt(dx*dx + dy*dy) - (body[skip] + body[i])); a NaN term never wins; a table without
    another row gives +inf."""
    tab = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    A = px.shape[0]
    if tab.shape[0] == 0:
        return np.full(A, np.inf)
    body = np.asarray(body, dtype=np.float64)
    skip = np.asarray(skip)
    dx = px[:, None] - tab[None, :, 0]
    dy = py[:, None] - tab[None, :, 1]
    with np.errstate(invalid="ignore"):
        both = body[skip][:, None] + body[None, :]
        cl = np.sqrt(dx * dx + dy * dy) - both
    cl = np.where(np.isnan(cl) | (np.arange(tab.shape[0])[None, :] == skip[:, None]), np.inf, cl)
    return cl.min(1)


class Metrics(sim_oracle.Metrics):
    """sim_oracle.Metrics with d_agent the clearance between bodies and collide_cycle; the obstacle half that of
    sizes_oracle.Metrics with a radius table, else sim_oracle's (centre distances, 0.5 m)."""

    def __init__(self, body, radius=None, c_first=0):
        super().__init__(c_first)
        self.body = np.asarray(body, dtype=np.float64)
        self.radius = None if radius is None else np.asarray(radius, dtype=np.float64)

    def update(self, c, state, obstacles, nbr_state, agent_offset=0):
        st = np.asarray(state, dtype=np.float64).reshape(-1, 4)
        px, py = st[:, 0], st[:, 2]
        A = st.shape[0]
        ob = np.zeros((0, 2)) if obstacles is None else obstacles
        self.d_obs = sim_oracle.nearest(px, py, ob) if self.radius is None else sizes_oracle.clearance(px, py, ob, self.radius)
        self.d_agent = body_clearance(px, py, np.zeros((0, 4)) if nbr_state is None else nbr_state, self.body,
                                      agent_offset + np.arange(A))
        if c == self.c_first:
            self.min_d_obs, self.min_d_agent = self.d_obs.copy(), self.d_agent.copy()
            self.fail_cycle = np.full(A, -1, np.int32)
            self.collide_cycle = np.full(A, -1, np.int32)
            self.distance_to_fail = np.zeros(A)
        else:
            self.min_d_obs = np.where(self.d_obs < self.min_d_obs, self.d_obs, self.min_d_obs)
            self.min_d_agent = np.where(self.d_agent < self.min_d_agent, self.d_agent, self.min_d_agent)
        hit = (self.fail_cycle < 0) & (self.d_obs < (0.5 if self.radius is None else 0.0))
        self.fail_cycle = np.where(hit, c, self.fail_cycle).astype(np.int32)
        self.distance_to_fail = np.where(hit, np.sqrt(px * px + py * py), self.distance_to_fail)
        self.collide_cycle = np.where((self.collide_cycle < 0) & (self.d_agent < 0.0), c, self.collide_cycle).astype(np.int32)
        return self

    def as_dict(self):
        return dict(super().as_dict(), collide_cycle=self.collide_cycle)


# ---------------------------------------------------------------------------- shared references (read-only)
_cache = {}


def tables(shape):
    """workload.agent_sizes for the neighbour table of one of plan_oracle.SHAPES (seed: the shape's)."""
    n_all = plan_oracle.reference(shape)["b"]["nbr_state"].shape[0]
    return workload.agent_sizes(n_all, shape[5])


def reference(shape, what):
    """For one of plan_oracle.SHAPES, computed once per `what`: the oracle's answer with the drawn tables --
    "rad", "pad", "both"; "sel_c" the clearance selection [A][Ko + Kn] (static columns the oracle's own) and "clear"
    the answer with both tables handed that selection; "moving" both tables beside workload.obstacle_sizes' levels
    and moving_oracle's velocities; "plan" both tables against plan_oracle's plan table."""
    key = (shape, what)
    if key not in _cache:
        R = plan_oracle.reference(shape)
        b, p = R["b"], R["p"]
        rad, pad, _ = tables(shape)
        if what == "sel_c":
            r = full_sel(p, b, nbr_clear_select(b["x0"], b["nbr_state"], rad, shape[3]))
        elif what == "clear":
            r = solve(p, b, rad, pad, sel=reference(shape, "sel_c"))
        elif what == "moving":
            r = solve(p, b, rad, pad, obs_eps=sizes_oracle.reference(shape)["eps"], vel=moving_oracle.reference(shape)["vel"])
        elif what == "plan":
            r = solve(p, b, rad, pad, table=R["table"])
        else:
            r = solve(p, b, rad if what in ("rad", "both") else None, pad if what in ("pad", "both") else None)
        for v in (r.values() if isinstance(r, dict) else (r,)):
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def world(run):
    """Start state, goals, obstacles and the agent tables (rad, pad, body) of one of RUNS."""
    state, goal, ob, _ = moving_oracle.world(run)
    return (state, goal, ob) + workload.agent_sizes(state.shape[0], run[6])


_loops = {}


def closed_loop(run, clear=False):
    """The oracle-only closed loop of one of RUNS (static obstacles of one size) with the drawn agent tables,
    computed once: per cycle the agents' advance, the metrics with bodies, the solve with rad and pad (clear: the
    neighbour columns by clearance).  dict(status [T][A][2], traj [T+1][A][4], x [T][A][nv], metrics)."""
    key = (run, clear)
    if key not in _loops:
        A, N, C, Ko, Kn, T, seed = run
        p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
        st, goal, ob, rad, pad, body = world(run)
        traj, status, xs = [st], [], []
        m = Metrics(body)
        for c in range(T):
            b, _ = sim_oracle.cycle_inputs(p, st, goal, ob, c)
            m.update(c, st, ob, b["nbr_state"])
            sel = full_sel(p, b, nbr_clear_select(b["x0"], b["nbr_state"], rad, Kn)) if clear and Kn > 0 else None
            r = solve(p, b, rad, pad, sel=sel)
            status.append(r["status"]); xs.append(r["x"])
            st = sim_oracle.next_state(r["x"])
            traj.append(st)
        _loops[key] = dict(status=np.array(status), traj=np.array(traj), x=np.array(xs), metrics=m.as_dict())
    return _loops[key]
