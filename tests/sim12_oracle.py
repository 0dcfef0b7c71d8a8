"""numpy restatement of the SRB-12 rollout kernel (csrc/srb12_sim.hip) and the closed loop built on it.

advance12() is srb12_sim_advance_kernel: the solver inputs of a cycle rebuilt from the 12-state that starts it --
the goal-directed reference line of the LIP rollout (tests/sim_oracle.py), the height, a yaw reference that turns
towards the goal by at most yaw_step a cycle, the default stance rotated by that yaw, and the contact flags.  Every
expression keeps the kernel's grouping (the kernel is compiled with contraction off); sqrt, division and rint round
correctly on both sides, atan2, cos and sin do not, so everything is bitwise equal to the device except yaw_ref,
xref[..., 5] and foot[..., 0:2], which agree to a few ulp (TRIG_TOL).  The metrics are sim_oracle.Metrics on the
`com` rows.

closed_loop12() runs advance12 + metrics + oracle.solve_batch12 for T cycles: the oracle-only closed loop.
"""
import numpy as np

import sim_oracle
from srbnmpc import workload

NDOMAIN = 4
STANCE = sim_oracle.STANCE                                  # [4][2] FR FL RR RL
TRIG_TOL = 1e-12      # a few ulp of values below 100 m are under 1e-13


def next_state12(x):
    """[A][12] at the domain's end: X at grid index 3 of the decision vectors x [A][24N+1]."""
    return np.array(np.asarray(x)[:, 12 * (NDOMAIN - 1):12 * NDOMAIN], dtype=np.float64)


def advance12(N, Ts, state, goal, vref, c, phase=None, gait="trot", hcom=workload.HCOM12, yaw_step=0.1,
              hold_radius=0.05):
    """Solver inputs of cycle c from the state [A][12] and the goals [A][2]: dict(x0 [A,12], xref [A,N,12],
    foot [A,N,4,3], contact [A,N,4] int32, last_state [A,4] (x, y, xdot, ydot), com [A,4] (x, xdot, y, ydot),
    yaw_ref [A])."""
    st = np.asarray(state, dtype=np.float64).reshape(-1, 12)
    goal = np.asarray(goal, dtype=np.float64).reshape(-1, 2)
    A = st.shape[0]
    px, py, yaw, vx, vy = st[:, 0], st[:, 1], st[:, 5], st[:, 6], st[:, 7]
    dx, dy = goal[:, 0] - px, goal[:, 1] - py
    dist = np.sqrt(dx * dx + dy * dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        ux = np.where(dist > 0.0, dx / dist, 0.0)
        uy = np.where(dist > 0.0, dy / dist, 0.0)
        q = dist / (Ts * float(N))
        v = np.where(q < vref, q, vref)
        wx, wy = ux * v, uy * v
        two_pi = 2.0 * 3.141592653589793
        e = np.arctan2(dy, dx) - yaw
        e = e - two_pi * np.rint(e / two_pi)
        e = np.where(e > yaw_step, yaw_step, np.where(e < -yaw_step, -yaw_step, e))
        yaw_ref = np.where(dist > hold_radius, yaw + e, yaw)
        cs, sn = np.cos(yaw_ref), np.sin(yaw_ref)
    xref = np.zeros((A, N, 12))
    foot = np.zeros((A, N, 4, 3))
    contact = np.zeros((A, N, 4), np.int32)
    par0 = c + (np.zeros(A, np.int64) if phase is None else np.asarray(phase, dtype=np.int64))
    for k in range(N):
        t = Ts * float(k + 1)
        xref[:, k, 0] = px + wx * t
        xref[:, k, 1] = py + wy * t
        xref[:, k, 2] = hcom
        xref[:, k, 5] = yaw_ref
        xref[:, k, 6] = wx
        xref[:, k, 7] = wy
        j = k // NDOMAIN
        tj = Ts * float(NDOMAIN * j)
        cx, cy = px + wx * tj, py + wy * tj
        odd = ((par0 + j) & 1) != 0
        for l in range(4):
            sx, sy = STANCE[l, 0], STANCE[l, 1]
            foot[:, k, l, 0] = cx + (cs * sx - sn * sy)
            foot[:, k, l, 1] = cy + (sn * sx + cs * sy)
            contact[:, k, l] = 1 if gait == "stand" else ((l in (0, 3)) != odd)
    return dict(x0=st.copy(), xref=xref, foot=foot, contact=contact, last_state=np.stack([px, py, vx, vy], 1),
                com=np.stack([px, vx, py, vy], 1), yaw_ref=yaw_ref)


# ---- the runs of the closed-loop tests: (A, N, gait, seed, T, K_obs, K_nbr)
RUNS12 = [(12, 10, "trot", 5, 8, 3, 4), (12, 10, "stand", 5, 8, 3, 4), (8, 4, "trot", 6, 8, 1, 2),
          (8, 6, "stand", 7, 6, 1, 0)]


def team12(A, N, gait, seed):
    """Start state [A][12], goals [A][2], obstacles and phases [A] int32 of a run: workload.make_batch12's states
    and obstacles, every goal at GOAL * (arena_scale, 1), except agent 0 (at rest at its goal), agent 1 (at rest,
    its goal 3 cm ahead in x) and agent 2 (its goal at start - (3, 1): behind it, so its yaw reference runs into
    the clamp and the bearing error into the wrap); phases from default_rng(seed).integers(0, 4, A)."""
    b = workload.make_batch12(A, N, gait, seed=seed)
    state = np.array(b["x0"], dtype=np.float64)
    goal = np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1))
    state[0, 6:12] = 0.0
    goal[0] = state[0, 0:2]
    state[1, 6:12] = 0.0
    goal[1] = state[1, 0:2] + np.array([0.03, 0.0])
    goal[2] = state[2, 0:2] - np.array([3.0, 1.0])
    phase = np.random.default_rng(seed).integers(0, 4, A).astype(np.int32)
    return state, goal, np.array(b["obstacles"], dtype=np.float64), phase


def cycle_inputs12(p, state, goal, obstacles, c, phase, gait):
    """The batch dict of cycle c from the cycle's start state (the rollout's wiring: the snapshot rows are the
    neighbour table)."""
    b = advance12(p.N, p.Ts, state, goal, workload.VREF, c, phase, gait)
    b["obstacles"] = obstacles
    b["nbr_state"] = b["last_state"]
    return b


def solve12(p, b):
    import oracle
    return oracle.solve_batch12(p, b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], b["nbr_state"])


def com_of(state):
    st = np.asarray(state)
    return np.stack([st[:, 0], st[:, 6], st[:, 1], st[:, 7]], 1)


_loops = {}


def closed_loop12(run):
    """The oracle-only closed loop of one of RUNS12, computed once (read-only): dict(p, state0, goal, obstacles,
    phase, traj [T+1][A][12], status [T][A][2], x [T][A][24N+1], metrics (the final dict))."""
    if run not in _loops:
        import oracle
        A, N, gait, seed, T, Ko, Kn = run
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        state0, goal, obstacles, phase = team12(A, N, gait, seed)
        st = state0
        traj, status, xs = [st], [], []
        m = sim_oracle.Metrics(0)
        for c in range(T):
            b = cycle_inputs12(p, st, goal, obstacles, c, phase, gait)
            m.update(c, b["com"], obstacles, b["nbr_state"])
            r = solve12(p, b)
            status.append(r["status"]); xs.append(r["x"])
            st = next_state12(r["x"])
            traj.append(st)
        out = dict(p=p, state0=state0, goal=goal, obstacles=obstacles, phase=phase, traj=np.array(traj),
                   status=np.array(status), x=np.array(xs), metrics=m.as_dict())
        for v in list(out.values()) + list(out["metrics"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _loops[run] = out
    return _loops[run]
