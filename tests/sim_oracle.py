"""numpy restatement of the rollout kernels (csrc/srb_sim.hip), bit for bit, and the closed loop built on it.

advance() is srb_sim_advance_kernel: the state that starts a cycle (the caller's, or X at grid index 3 of the
previous solution), the solver inputs rebuilt from it -- the goal-directed reference and trot footholds of
workload.make_batch re-centred on the current position -- and last cycle's plans shifted by one gait domain.
metrics() / Metrics is srb_sim_metrics_kernel.  Every expression keeps the kernel's grouping (the kernel is
compiled with contraction off), numpy's sqrt and division round correctly as the device's do, and a minimum is
exact in any order, so the comparison with the device is assert_array_equal.

closed_loop() runs advance + metrics + plan_oracle.solve for T cycles: the oracle-only closed loop.
"""
import numpy as np

import plan_oracle
from srbnmpc import workload

NDOMAIN = 4
STANCE = np.array([[0.2188, -0.1320], [0.2188, 0.1320], [-0.1472, -0.1320], [-0.1472, 0.1320]])   # FR FL RR RL


def next_state(x):
    """[A][4] x, xdot, y, ydot at the domain's end: X at grid index 3 of the decision vectors x [A][nv]."""
    return np.array(np.asarray(x)[:, 4 * (NDOMAIN - 1):4 * NDOMAIN], dtype=np.float64)


def shift4(N, x):
    """The plan table [A][N][2] of the next cycle from decision vectors x [A][nv] (dist.shift_plans(., 4))."""
    X = np.asarray(x)[:, :4 * N].reshape(-1, N, 4)
    P = X[:, :, [0, 2]]
    out = np.empty((P.shape[0], N, 2))
    last, e = P[:, N - 1], P[:, N - 1] - P[:, N - 2]
    for k in range(N):
        if k + NDOMAIN < N:
            out[:, k] = P[:, k + NDOMAIN]
        else:
            out[:, k] = last + float(k + NDOMAIN - N + 1) * e
    return out


def advance(N, C, Ts, state, goal, vref, c, phase=None):
    """Solver inputs of cycle c from the state [A][4] (x, xdot, y, ydot) and the goals [A][2]:
    dict(x0 [A,4], ref [A,4N], foot [A,N,2,C], last_state [A,4])."""
    st = np.asarray(state, dtype=np.float64).reshape(-1, 4)
    goal = np.asarray(goal, dtype=np.float64).reshape(-1, 2)
    A = st.shape[0]
    px, vx, py, vy = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    dx, dy = goal[:, 0] - px, goal[:, 1] - py
    dist = np.sqrt(dx * dx + dy * dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        ux = np.where(dist > 0.0, dx / dist, 0.0)
        uy = np.where(dist > 0.0, dy / dist, 0.0)
    q = dist / (Ts * float(N))
    v = np.where(q < vref, q, vref)
    wx, wy = ux * v, uy * v
    ref = np.zeros((A, N, 4))
    for k in range(N):
        t = Ts * float(k + 1)
        ref[:, k, 0] = px + wx * t
        ref[:, k, 1] = wx
        ref[:, k, 2] = py + wy * t
        ref[:, k, 3] = wy
    par0 = c + (np.zeros(A, np.int64) if phase is None else np.asarray(phase, dtype=np.int64))
    foot = np.zeros((A, N, 2, C))
    for k in range(N):
        j = k // NDOMAIN
        t = Ts * float(NDOMAIN * j)
        cx, cy = px + wx * t, py + wy * t
        odd = ((par0 + j) & 1) != 0
        for i in range(C):
            leg = np.where(odd, 1 + i, 3 * i) if C == 2 else np.full(A, i)
            foot[:, k, 0, i] = STANCE[leg, 0] + cx
            foot[:, k, 1, i] = STANCE[leg, 1] + cy
    return dict(x0=st.copy(), ref=ref.reshape(A, 4 * N), foot=foot, last_state=np.stack([px, py, vx, vy], 1))


def nearest(px, py, table, skip=None):
    """sqrt of the smallest dx*dx + dy*dy over the rows of table [n][>= 2] (columns 0, 1); skip [A]: the row
    each agent leaves out.  A NaN never wins; an empty table gives +inf."""
    tab = np.asarray(table, dtype=np.float64)
    tab = tab.reshape(-1, tab.shape[-1] if tab.ndim > 1 else 2)
    A = px.shape[0]
    if tab.shape[0] == 0:
        return np.full(A, np.inf)
    dx = px[:, None] - tab[None, :, 0]
    dy = py[:, None] - tab[None, :, 1]
    d2 = dx * dx + dy * dy
    d2 = np.where(np.isnan(d2), np.inf, d2)
    if skip is not None:
        rows = np.arange(tab.shape[0])[None, :]
        d2 = np.where(rows == np.asarray(skip)[:, None], np.inf, d2)
    return np.sqrt(d2.min(1))


class Metrics:
    """The running safety metrics of srb_sim_metrics_kernel over the cycles fed to update()."""

    def __init__(self, c_first=0):
        self.c_first = c_first

    def update(self, c, state, obstacles, nbr_state, agent_offset=0):
        st = np.asarray(state, dtype=np.float64).reshape(-1, 4)
        px, py = st[:, 0], st[:, 2]
        A = st.shape[0]
        self.d_obs = nearest(px, py, np.zeros((0, 2)) if obstacles is None else obstacles)
        self.d_agent = nearest(px, py, np.zeros((0, 4)) if nbr_state is None else nbr_state, agent_offset + np.arange(A))
        if c == self.c_first:
            self.min_d_obs, self.min_d_agent = self.d_obs.copy(), self.d_agent.copy()
            self.fail_cycle = np.full(A, -1, np.int32)
            self.distance_to_fail = np.zeros(A)
        else:
            self.min_d_obs = np.where(self.d_obs < self.min_d_obs, self.d_obs, self.min_d_obs)
            self.min_d_agent = np.where(self.d_agent < self.min_d_agent, self.d_agent, self.min_d_agent)
        hit = (self.fail_cycle < 0) & (self.d_obs < 0.5)
        self.fail_cycle = np.where(hit, c, self.fail_cycle).astype(np.int32)
        self.distance_to_fail = np.where(hit, np.sqrt(px * px + py * py), self.distance_to_fail)
        return self

    def as_dict(self):
        return {k: getattr(self, k) for k in ("d_obs", "d_agent", "min_d_obs", "min_d_agent", "fail_cycle",
                                              "distance_to_fail")}


# ---- the runs of the issue's "Conditions checked here": (A, N, C, K_obs, K_nbr, T, seed, plans)
RUNS = [(16, 10, 2, 3, 4, 8, 5, False), (16, 10, 2, 3, 4, 8, 5, True), (12, 4, 2, 1, 2, 8, 6, True),
        (8, 4, 4, 1, 0, 6, 7, False)]


def team(A, N, C, seed):
    """Start state [A][4], goals [A][2] and obstacles of a run: workload.make_batch's positions, velocities and
    obstacles, every goal at GOAL * (arena_scale, 1), except agent 0 (standing at its goal) and agent 1 (at
    rest, its goal 0.03, 0.02 m from its start)."""
    b = workload.make_batch(A, N, C, seed=seed)
    state = np.array(b["x0"], dtype=np.float64)
    goal = np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1))
    state[0, 1] = state[0, 3] = 0.0
    goal[0] = state[0, [0, 2]]
    state[1, 1] = state[1, 3] = 0.0
    goal[1] = state[1, [0, 2]] + np.array([0.03, 0.02])
    return state, goal, np.array(b["obstacles"], dtype=np.float64)


def cycle_inputs(p, state, goal, obstacles, c, x_prev=None, plans=False, phase=None):
    """The batch dict of cycle c and its plan table (None: constant velocity) from the cycle's start state."""
    b = advance(p.N, p.C, p.Ts, state, goal, workload.VREF, c, phase)
    b["obstacles"] = obstacles
    b["nbr_state"] = b["last_state"]
    table = shift4(p.N, x_prev) if (plans and x_prev is not None) else None
    return b, table


_loops = {}


def closed_loop(run):
    """The oracle-only closed loop of one of RUNS, computed once (read-only): dict(p, state0, goal, obstacles,
    traj [T+1][A][4], status [T][A][2], x [T][A][nv], metrics (the final dict), fail_cycle)."""
    if run not in _loops:
        import oracle
        A, N, C, Ko, Kn, T, seed, plans = run
        p = oracle.params(N, C, K_obs=Ko, K_nbr=Kn)
        state0, goal, obstacles = team(A, N, C, seed)
        st, xp = state0, None
        traj, status, xs = [st], [], []
        m = Metrics(0)
        for c in range(T):
            b, table = cycle_inputs(p, st, goal, obstacles, c, xp, plans)
            m.update(c, st, obstacles, b["nbr_state"])
            r = plan_oracle.solve(p, b, table)
            status.append(r["status"]); xs.append(r["x"])
            xp, st = r["x"], next_state(r["x"])
            traj.append(st)
        out = dict(p=p, state0=state0, goal=goal, obstacles=obstacles, traj=np.array(traj), status=np.array(status),
                   x=np.array(xs), metrics=m.as_dict())
        for v in list(out.values()) + list(out["metrics"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _loops[run] = out
    return _loops[run]
