"""The reference answers for obstacle sizes (srb_sizes), from the oracle's own pieces and numpy.

solve() is moving_oracle.solve_agent's chain -- QP build, QP stage at the warm-start tolerance, selection, NLP stage
warm-started from the QP point -- with eps[:K_obs], the levels oracle.nlp_solve takes per column, overwritten by
obs_eps[idx[j]].  With a table that holds eps_obs in every row it is oracle.solve_batch bit for bit
(tests/test_obstacle_sizes.py pins that).

clearance_keys() / clearance_select() restate srb_knn_obs_clear_kernel: the key sqrt(m) - sqrt(obs_eps[i]) with m the
squared distance now, or with a velocity table moving_oracle.horizon_keys' minimum over the horizon; a stable sort on
(key, index), NaN keys never selected, and the static table's 1000 m rule on the key (moving_oracle.select_by_key).
numpy neither fuses a multiply-add nor reorders a sum and its sqrt rounds correctly, so the comparison with the device
is index for index.  Metrics is srb_sim_metrics_sized_kernel, bit for bit.

closed_loop() is the oracle-only closed loop with sizes, static or moving, on sim_oracle's advance and next_state.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import moving_oracle
import oracle
import plan_oracle
import sim_oracle
from srbnmpc import workload

RUNS = moving_oracle.RUNS


def solve_agent(p, x0, ref, foot, obstacles, obs_eps, vel, nbr_state, table, self_idx, idx=None):
    """moving_oracle.solve_agent with the levels of the static columns taken from obs_eps [n_obs] (vel None: static
    obstacles).  p is already clamped.  Returns x_qp, x, obj, status[2], iters[2], idx."""
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
        eps[:p.K_obs] = np.asarray(obs_eps, dtype=np.float64)[rows]
    if table is None and given and p.K_nbr > 0:
        table = plan_oracle.cv_table(p, nbr_state)          # the oracle's own rows, bit for bit, for the given idx
    if table is not None:
        for j in range(p.K_obs, p.K_obs + p.K_nbr):
            if idx[j] >= 0:
                obs[:, j, :] = table[idx[j]]
    x, st1, it1 = oracle.nlp_solve(p, x0, foot, Pd, c, A, b, G, h, obs, eps, xq)
    obj = float(np.sum(0.5 * Pd * x * x + c * x))
    return xq, x, obj, (st0, st1), (it0.value, it1), np.asarray(idx, np.int32)


def solve(p, batch, obs_eps, vel=None, sel=None, table=None, agent_offset=0):
    """The batch (workload.make_batch's dict) against obstacles of levels obs_eps [n_obs], moving at vel or static."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    A = x0.shape[0]
    ref = np.asarray(batch["ref"]).reshape(A, -1)
    foot = np.asarray(batch["foot"]).reshape(A, -1)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = plan_oracle.clamped(p, ob.shape[0], nb.shape[0])
    oracle.lib().orc_qp_solve_init.restype = ctypes.c_int

    def one(a):
        return solve_agent(q, x0[a], ref[a], foot[a], ob, obs_eps, vel, nb, table, agent_offset + a,
                           None if sel is None else sel[a])
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(A)))
    return dict(x_qp=np.array([r[0] for r in res]), x=np.array([r[1] for r in res]),
                obj=np.array([r[2] for r in res]), status=np.array([r[3] for r in res], np.int32),
                iters=np.array([r[4] for r in res], np.int32), sel=np.array([r[5] for r in res], np.int32))


# ---------------------------------------------------------------------------- clearance selection
def clearance_keys(x0, ob, obs_eps, Ts=0.0, N=0, vel=None):
    """[A][n_obs]: sqrt(m) - sqrt(obs_eps), m the squared distance now (vel None) or the horizon's minimum; NaN
    where the row, its velocity or its level is NaN, or the level negative."""
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    d = moving_oracle.snapshot_keys(x0, ob) if vel is None else moving_oracle.horizon_keys(Ts, N, x0, ob, vel)
    with np.errstate(invalid="ignore"):
        return d - np.sqrt(np.asarray(obs_eps, dtype=np.float64))[None]


def clearance_select(x0, ob, obs_eps, K, Ts=0.0, N=0, vel=None, scene_agents=0, scene_obs=0, agent_offset=0):
    """The static columns of srb_knn_obs_clear_kernel; with scenes, of its scene form (global indices)."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 4)
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    obs_eps = np.asarray(obs_eps, dtype=np.float64)
    if scene_agents <= 0:
        return moving_oracle.select_by_key(clearance_keys(x0, ob, obs_eps, Ts, N, vel), K)
    rows = []
    for a in range(x0.shape[0]):
        o0 = ((agent_offset + a) // scene_agents) * scene_obs
        v = None if vel is None else np.asarray(vel)[o0:o0 + scene_obs]
        key = clearance_keys(x0[a:a + 1], ob[o0:o0 + scene_obs], obs_eps[o0:o0 + scene_obs], Ts, N, v)
        rows.append(moving_oracle.select_by_key(key, K, o0)[0])
    return np.array(rows, np.int32)


def full_sel(p, batch, static_cols):
    """[A][Ko + Kn]: static_cols beside the oracle's own neighbour columns."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = plan_oracle.clamped(p, ob.shape[0], nb.shape[0])
    snap = np.array([oracle.select_idx(q, x0[a], ob, nb, a) for a in range(x0.shape[0])], np.int32)
    return np.concatenate([np.asarray(static_cols, np.int32), snap[:, q.K_obs:]], 1)


# ---------------------------------------------------------------------------- metrics
def clearance(px, py, table, radius):
    """min_i (sqrt(dx*dx + dy*dy) - radius[i]); a NaN term never wins; an empty table gives +inf."""
    tab = np.asarray(table, dtype=np.float64).reshape(-1, 2)
    if tab.shape[0] == 0:
        return np.full(px.shape[0], np.inf)
    dx = px[:, None] - tab[None, :, 0]
    dy = py[:, None] - tab[None, :, 1]
    with np.errstate(invalid="ignore"):
        cl = np.sqrt(dx * dx + dy * dy) - np.asarray(radius, dtype=np.float64)[None]
    return np.where(np.isnan(cl), np.inf, cl).min(1)


class Metrics(sim_oracle.Metrics):
    """sim_oracle.Metrics with d_obs the clearance to the bodies and the fail test d_obs < 0."""

    def __init__(self, radius, c_first=0):
        super().__init__(c_first)
        self.radius = np.asarray(radius, dtype=np.float64)

    def update(self, c, state, obstacles, nbr_state, agent_offset=0):
        st = np.asarray(state, dtype=np.float64).reshape(-1, 4)
        px, py = st[:, 0], st[:, 2]
        A = st.shape[0]
        self.d_obs = clearance(px, py, np.zeros((0, 2)) if obstacles is None else obstacles, self.radius)
        self.d_agent = sim_oracle.nearest(px, py, np.zeros((0, 4)) if nbr_state is None else nbr_state,
                                          agent_offset + np.arange(A))
        if c == self.c_first:
            self.min_d_obs, self.min_d_agent = self.d_obs.copy(), self.d_agent.copy()
            self.fail_cycle = np.full(A, -1, np.int32)
            self.distance_to_fail = np.zeros(A)
        else:
            self.min_d_obs = np.where(self.d_obs < self.min_d_obs, self.d_obs, self.min_d_obs)
            self.min_d_agent = np.where(self.d_agent < self.min_d_agent, self.d_agent, self.min_d_agent)
        hit = (self.fail_cycle < 0) & (self.d_obs < 0.0)
        self.fail_cycle = np.where(hit, c, self.fail_cycle).astype(np.int32)
        self.distance_to_fail = np.where(hit, np.sqrt(px * px + py * py), self.distance_to_fail)
        return self


# ---------------------------------------------------------------------------- shared references (read-only)
_cache = {}


def reference(shape):
    """For one of plan_oracle.SHAPES, computed once: plan_oracle.reference's batch, params and answer r0, the drawn
    table workload.obstacle_sizes(n_obs, seed), the sized oracle's answer r (centres selected as ever), the clearance
    selection sel_c ([A][Ko + Kn]) and the sized oracle's answer rc handed that selection."""
    if shape not in _cache:
        R = plan_oracle.reference(shape)
        b, p = R["b"], R["p"]
        eps, radius = workload.obstacle_sizes(b["obstacles"].shape[0], shape[5])
        r = solve(p, b, eps)
        sel_c = full_sel(p, b, clearance_select(b["x0"], b["obstacles"], eps, shape[2]))
        rc = solve(p, b, eps, sel=sel_c)
        for d in (r, rc):
            for v in d.values():
                v.setflags(write=False)
        for v in (eps, radius, sel_c):
            v.setflags(write=False)
        _cache[shape] = dict(b=b, p=p, r0=R["r0"], eps=eps, radius=radius, r=r, sel_c=sel_c, rc=rc)
    return _cache[shape]


def world(run, vmax=1.0):
    """Start state, goals, obstacles, velocities, levels and radii of one of RUNS."""
    state, goal, ob, vel = moving_oracle.world(run, vmax)
    eps, radius = workload.obstacle_sizes(ob.shape[0], run[6])
    return state, goal, ob, vel, eps, radius


_loops = {}


def closed_loop(run, moving=False, clear=False):
    """The oracle-only closed loop of one of RUNS with the drawn sizes, computed once: per cycle the agents' advance,
    for c > 0 and a moving world the obstacles' advance, the sized metrics, the sized solve (clear: the static
    columns by clearance, over the horizon when the world moves as the device does with obs_horizon).
    dict(status [T][A][2], traj [T+1][A][4], x [T][A][nv], metrics)."""
    key = (run, moving, clear)
    if key not in _loops:
        A, N, C, Ko, Kn, T, seed = run
        p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
        st, goal, ob, vel, eps, radius = world(run)
        w = vel if moving else None
        traj, status, xs = [st], [], []
        m = Metrics(radius, 0)
        for c in range(T):
            b, _ = sim_oracle.cycle_inputs(p, st, goal, ob, c)
            if c > 0 and moving:
                ob = moving_oracle.advance_obstacles(p.Ts, ob, vel)
                b["obstacles"] = ob
            m.update(c, st, ob, b["nbr_state"])
            sel = None
            if clear:
                sel = full_sel(p, b, clearance_select(b["x0"], ob, eps, Ko, p.Ts, N, w))
            r = solve(p, b, eps, w, sel=sel)
            status.append(r["status"]); xs.append(r["x"])
            st = sim_oracle.next_state(r["x"])
            traj.append(st)
        _loops[key] = dict(status=np.array(status), traj=np.array(traj), x=np.array(xs), metrics=m.as_dict())
    return _loops[key]
