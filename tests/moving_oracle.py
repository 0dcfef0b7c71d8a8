"""The reference answers for moving obstacles (srb_moving), from the oracle's own pieces and numpy.

solve() is plan_oracle.solve_agent's chain -- QP build, QP stage at the warm-start tolerance, selection, NLP stage
warm-started from the QP point -- with the static columns of the per-grid obstacle rows obs[N][K][2] that
oracle.nlp_solve takes overwritten by ob[idx[j]] + vel[idx[j]] * (Ts (k + 1)): the kernel's arithmetic, one rounded
multiply and one rounded add.  With a zero table it is oracle.solve_batch bit for bit
(tests/test_moving_obstacles.py pins that).

horizon_keys() / horizon_select() restate srb_knn_obs_horizon_kernel: the key sqrt(min over k = 0 .. N of
dx^2 + dy^2) with both points at constant velocity, a stable sort on (key, index), NaN rows never selected, and the
static table's 1000 m rule (a slot whose key is >= 1000, or that no row is left for, gets row 0).  numpy neither
fuses a multiply-add nor reorders a sum, and its sqrt rounds correctly, so the comparison with the device is
index for index.  advance_obstacles() is srb_obstacles_advance_kernel, bit for bit.

closed_loop() is the oracle-only closed loop with a moving table, on sim_oracle's advance, Metrics and next_state.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle
import plan_oracle
import sim_oracle
from srbnmpc import workload

# the closed-loop runs of the issue: (A, N, C, K_obs, K_nbr, T, seed), vmax 1.0, no plans
RUNS = [(16, 10, 2, 3, 4, 8, 5), (12, 4, 2, 1, 2, 8, 6), (8, 4, 4, 1, 0, 6, 7), (12, 20, 2, 3, 4, 6, 8)]


def moved_rows(p, ob, vel, rows):
    """[N][len(rows)][2]: obstacle rows `rows` at the grid times Ts (k + 1)."""
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    out = np.empty((p.N, len(rows), 2))
    for k in range(p.N):
        out[k] = ob[rows] + vel[rows] * (p.Ts * (k + 1))
    return out


def solve_agent(p, x0, ref, foot, obstacles, vel, nbr_state, table, self_idx, idx=None):
    """plan_oracle.solve_agent with the static columns moved by vel [n_obs][2].  idx: the selected rows to use
    instead of the oracle's snapshot selection; table: the neighbours' plan table [n_all][N][2] (None: constant
    velocity).  p is already clamped.  Returns x_qp, x, obj, status[2], iters[2], idx."""
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
    obs = np.array(obs, copy=True)
    if p.K_obs > 0:
        obs[:, :p.K_obs, :] = moved_rows(p, obstacles, vel, np.asarray(idx[:p.K_obs]))
    if table is None and given and p.K_nbr > 0:
        table = plan_oracle.cv_table(p, nbr_state)          # the oracle's own rows, bit for bit, for the given idx
    if table is not None:
        for j in range(p.K_obs, p.K_obs + p.K_nbr):
            if idx[j] >= 0:
                obs[:, j, :] = table[idx[j]]
    x, st1, it1 = oracle.nlp_solve(p, x0, foot, Pd, c, A, b, G, h, obs, eps, xq)
    obj = float(np.sum(0.5 * Pd * x * x + c * x))
    return xq, x, obj, (st0, st1), (it0.value, it1), np.asarray(idx, np.int32)


def solve(p, batch, vel, sel=None, table=None, agent_offset=0):
    """The batch (workload.make_batch's dict) against obstacles moving at vel [n_obs][2]."""
    x0 = np.asarray(batch["x0"]).reshape(-1, 4)
    A = x0.shape[0]
    ref = np.asarray(batch["ref"]).reshape(A, -1)
    foot = np.asarray(batch["foot"]).reshape(A, -1)
    ob = np.asarray(batch["obstacles"]).reshape(-1, 2)
    nb = np.asarray(batch["nbr_state"]).reshape(-1, 4)
    q = plan_oracle.clamped(p, ob.shape[0], nb.shape[0])
    oracle.lib().orc_qp_solve_init.restype = ctypes.c_int

    def one(a):
        return solve_agent(q, x0[a], ref[a], foot[a], ob, vel, nb, table, agent_offset + a, None if sel is None else sel[a])
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(A)))
    return dict(x_qp=np.array([r[0] for r in res]), x=np.array([r[1] for r in res]),
                obj=np.array([r[2] for r in res]), status=np.array([r[3] for r in res], np.int32),
                iters=np.array([r[4] for r in res], np.int32), sel=np.array([r[5] for r in res], np.int32))


# ---------------------------------------------------------------------------- horizon-aware obstacle selection
def horizon_keys(Ts, N, x0, ob, vel):
    """[A][n_obs]: sqrt(min_k d_k^2), k = 0 .. N, t_k = Ts * float(k); NaN where any pair is NaN."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 4)
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    t = np.array([Ts * float(k) for k in range(N + 1)])
    px = x0[:, 0, None] + x0[:, 1, None] * t[None]
    py = x0[:, 2, None] + x0[:, 3, None] * t[None]
    with np.errstate(invalid="ignore", over="ignore"):
        ox = ob[:, 0, None] + vel[:, 0, None] * t[None]
        oy = ob[:, 1, None] + vel[:, 1, None] * t[None]
        dx = px[:, None, :] - ox[None]
        dy = py[:, None, :] - oy[None]
        d2 = dx * dx + dy * dy
        return np.sqrt(np.min(d2, axis=2))                  # np.min propagates NaN


def snapshot_keys(x0, ob):
    """The key of the snapshot selection: the distance now."""
    return horizon_keys(0.0, 0, x0, ob, np.zeros_like(np.asarray(ob, dtype=np.float64).reshape(-1, 2)))


def select_by_key(key, K, base=0):
    """[A][min(K, n)]: rows in (key, index) order, NaN rows never, a slot with key >= 1000 or no row left: row 0."""
    A, n = key.shape
    K = min(K, n)
    out = np.zeros((A, K), np.int32)
    for a in range(A):
        order = [i for i in np.lexsort((np.arange(n), key[a])) if not np.isnan(key[a, i])]
        for j in range(K):
            out[a, j] = order[j] if j < len(order) and key[a, order[j]] < 1000.0 else 0
    return out + base


def horizon_select(Ts, N, x0, ob, vel, K, scene_agents=0, scene_obs=0, agent_offset=0):
    """The static columns of srb_knn_obs_horizon_kernel; with scenes, of its scene form (global indices)."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 4)
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    if scene_agents <= 0:
        return select_by_key(horizon_keys(Ts, N, x0, ob, vel), K)
    rows = []
    for a in range(x0.shape[0]):
        o0 = ((agent_offset + a) // scene_agents) * scene_obs
        rows.append(select_by_key(horizon_keys(Ts, N, x0[a:a + 1], ob[o0:o0 + scene_obs], vel[o0:o0 + scene_obs]), K, o0)[0])
    return np.array(rows, np.int32)


def advance_obstacles(Ts, ob, vel, cycles=1):
    """The table after `cycles` control cycles of 4 grids each."""
    ob = np.array(ob, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(cycles):
            ob = ob + vel * (Ts * 4.0)
    return ob


# ---------------------------------------------------------------------------- shared references (read-only)
_cache = {}


def reference(shape, vmax=1.0):
    """For one of plan_oracle.SHAPES, computed once: plan_oracle.reference's batch, params and static answer r0,
    the velocities workload.obstacle_velocities(n_obs, seed, vmax) and the moving oracle's answer r."""
    if (shape, vmax) not in _cache:
        R = plan_oracle.reference(shape)
        vel = workload.obstacle_velocities(R["b"]["obstacles"].shape[0], shape[5], vmax)
        r = solve(R["p"], R["b"], vel)
        for v in r.values():
            v.setflags(write=False)
        vel.setflags(write=False)
        _cache[(shape, vmax)] = dict(b=R["b"], p=R["p"], r0=R["r0"], vel=vel, r=r)
    return _cache[(shape, vmax)]


def world(run, vmax=1.0):
    """Start state, goals, obstacles and velocities of one of RUNS."""
    A, N, C, Ko, Kn, T, seed = run
    state, goal, ob = sim_oracle.team(A, N, C, seed)
    return state, goal, ob, workload.obstacle_velocities(ob.shape[0], seed, vmax)


def closed_loop(run, aware=True, vmax=1.0):
    """The oracle-only closed loop of one of RUNS in the moving world: per cycle the agents' advance, for c > 0 the
    obstacles' advance, the metrics on the moved table, the solve -- aware of the velocities, or (aware=False) the
    same moving world solved as if the table it re-reads every cycle were static.  dict(status [T][A][2],
    traj [T+1][A][4], obstacles (the last cycle's table), metrics)."""
    A, N, C, Ko, Kn, T, seed = run
    p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
    st, goal, ob, vel = world(run, vmax)
    traj, status = [st], []
    m = sim_oracle.Metrics(0)
    for c in range(T):
        b, _ = sim_oracle.cycle_inputs(p, st, goal, ob, c)
        if c > 0:
            ob = advance_obstacles(p.Ts, ob, vel)
            b["obstacles"] = ob
        m.update(c, st, ob, b["nbr_state"])
        r = solve(p, b, vel if aware else np.zeros_like(vel))
        status.append(r["status"])
        st = sim_oracle.next_state(r["x"])
        traj.append(st)
    return dict(status=np.array(status), traj=np.array(traj), obstacles=ob, metrics=m.as_dict())
