"""Restatements for the degraded neighbour link of the SRB-12 mode (srb12_link_update_device,
srb12_solve_batch_link_device, srb12_rollout_link_device; Rollout12(link=...)).

The link itself is tests/link_oracle.py, imported: the SRB-12 mode runs srb_link_update_kernel unchanged, with the
LIP layouts of the snapshot row and the plan tables.  What is new here:

  select_own    the horizon-aware selection with the agent's own plan from a table of its own: for agent g the existing
                restatement of the plan selection (test_nbr_plan.brute_force, the header's definition) on the perceived
                table with row g replaced by the truth row, agent g's columns kept.  With scene_agents the scan is the
                agent's scene alone, global indices out.
  linear_rows   (P, w) [n][2] each with table[i][k] = P_i + w_i * (Ts * (k + 1)) for a plan table whose rows are
                straight lines in k, and the largest departure of the table from that line.  At N = 4 EVERY plan table of
                a rollout is such a table: the shift between cycles moves a plan by 4 = N grids, so all of a shifted
                plan lies past the horizon, on the line through its last point along its last finite difference; a
                held plan is a copy of one, and dead reckoning by 4 age grids moves it further along the same line.
  solve_seen    the oracle's answer of one cycle for what the agents perceive: oracle.solve_batch12 predicts a
                neighbour at constant velocity from its snapshot row, p + v * (Ts * (k + 1)), so per agent it is called
                with the agent's selected rows alone, each as the snapshot (P_i, w_i) of its perceived line.  That is
                the problem the device solves up to the rounding of the line (a few ulp of a position, 1e-15 m: nine
                orders below X_TOL).  The selection handed over is the snapshot selection on the perceived positions
                (brute_force, horizon=False), the rule the selection tests pin bit for bit.
"""
import numpy as np

import link_oracle  # noqa: F401  (the link: tables, new_state, update, run)
import oracle
from conftest import converged  # noqa: F401  (QP OPTIMAL or QP_WARM, NLP OPTIMAL)
from test_nbr_plan import brute_force

LINE_TOL = 1e-12            # metres: a table row counts as a line when no grid is further from it


def lip_rows(x0):
    """[x, xdot, y, ydot] rows of 12-state x0 [A][12]: what the selection reads."""
    return np.ascontiguousarray(np.asarray(x0)[:, [0, 6, 1, 7]])


def select_own(x0, nbr, seen_plan, own_plan, Kn, lo=0, scene_agents=0):
    """Neighbour columns [A][Kn] (int32, -1: none) of agents lo .. lo + A - 1: x0 [A][4] (x, xdot, y, ydot), nbr
    [n_all][4] and seen_plan [n_all][N][2] the perceived tables, own_plan [A][N][2] the agents' own plans (indexed by
    the local agent).  own_plan None: the plain restatement (row g of seen_plan)."""
    x0, nbr, seen_plan = np.asarray(x0), np.asarray(nbr), np.asarray(seen_plan)
    A, n_all = x0.shape[0], nbr.shape[0]
    out = np.full((A, Kn), -1, np.int32)
    for a in range(A):
        g = lo + a
        base, rows = 0, n_all
        if scene_agents:
            base, rows = (g // scene_agents) * scene_agents, scene_agents
        table = np.array(seen_plan[base:base + rows])
        if own_plan is not None:
            table[g - base] = own_plan[a]
        r = brute_force(x0[a:a + 1], nbr[base:base + rows], table, Kn, lo=g - base, hi=g - base + 1)[0]
        out[a] = np.where(r >= 0, r + base, -1)
    return out


def linear_rows(table, Ts):
    """(P [n][2], w [n][2], err): the line of every row of table [n][N][2] through its first two grids, and the largest
    |table[i][k] - (P_i + w_i * (Ts * (k + 1)))|."""
    T = np.asarray(table, np.float64)
    N = T.shape[1]
    w = (T[:, 1] - T[:, 0]) / Ts
    P = T[:, 0] - w * Ts
    tt = np.array([Ts * (k + 1) for k in range(N)])
    line = P[:, None] + w[:, None] * tt[None, :, None]
    return P, w, float(np.abs(T - line).max())


def solve_seen(p, b, seen_state, seen_plan):
    """One cycle's oracle answers for the batch b (sim12_oracle.cycle_inputs12) against the perceived tables: dict x,
    status, iters [A].., sel [A][K_nbr] (the rows used) and line_err.  seen_plan None: the constant-velocity rows of
    seen_state itself (the first cycle, or plans off)."""
    seen_state = np.asarray(seen_state, np.float64)
    A, Kn = b["x0"].shape[0], p.K_nbr
    if seen_plan is None:
        P, w, err = seen_state[:, :2], seen_state[:, 2:], 0.0
    else:
        P, w, err = linear_rows(seen_plan, p.Ts)
    eq = np.concatenate([P, w], 1)
    sel = brute_force(lip_rows(b["x0"]), seen_state, None, min(Kn, A - 1), horizon=False)
    out = dict(x=[], status=[], iters=[])
    for a in range(A):
        assert (sel[a] >= 0).all()
        nbr = np.ascontiguousarray(np.concatenate([eq[a:a + 1], eq[sel[a]]]))     # row 0: the agent's own, left out
        r = oracle.solve_batch12(p, b["x0"][a:a + 1], b["xref"][a:a + 1], b["foot"][a:a + 1], b["contact"][a:a + 1],
                                 b["obstacles"], nbr, agent_offset=0, nthreads=1)
        for k in out:
            out[k].append(r[k][0])
    out = {k: np.array(v) for k, v in out.items()}
    out["sel"], out["line_err"] = sel, err
    return out


# ---- the closed loop of the link tests: (A, N, gait, seed, T, K_obs, K_nbr); every row two cycles late, a fifth of
# the broadcasts lost, positions off by up to 3 cm (test_link_gpu.degraded's tables)
LOOP = (8, 4, "trot", 6, 6, 1, 2)
LINK_SEED, DELAY, DROP, NOISE_P = 21, 2, 0.2, 0.03
GRID = 1.5            # metres between the starts: inside sqrt(eps_nbr) = 1.48 m within the first cycles


def head_on_team12(A, N, gait, seed):
    """workload.make_batch12's states, obstacles and phases with the starts on two rows of a GRID-metre grid that walk
    at each other: every goal lies straight across the other row, yaws and velocities turned to that bearing (the drawn
    speed kept).  test_plant12_gpu.spread_team12's 2.2 m grid keeps every pair beyond sqrt(eps_nbr) = 1.48 m, so its
    inter-agent rows are inactive and a perceived table changes nothing; here neighbours start 1.5 m apart and close
    in, the rows are active from the first cycles, and 3 cm on a neighbour's position moves the optimum by far more
    than the solve tolerances (chosen on the CPU oracle alone: test_link12.py runs that loop)."""
    from srbnmpc import workload
    b = workload.make_batch12(A, N, gait, seed=seed)
    state = np.array(b["x0"], dtype=np.float64)
    cols = (A + 1) // 2
    state[:, 0] = 0.4 + GRID * (np.arange(A) % cols)
    state[:, 1] = np.where(np.arange(A) < cols, -GRID / 2, GRID / 2)
    goal = np.stack([state[:, 0], -6.0 * state[:, 1]], 1)
    bearing = np.arctan2(goal[:, 1] - state[:, 1], goal[:, 0] - state[:, 0])
    speed = np.hypot(state[:, 6], state[:, 7])
    state[:, 5] = bearing
    state[:, 6], state[:, 7] = speed * np.cos(bearing), speed * np.sin(bearing)
    phase = np.random.default_rng(seed).integers(0, 4, A).astype(np.int32)
    return state, goal, np.array(b["obstacles"], dtype=np.float64), phase


def loop_tables(A, extrapolate, Ts):
    return link_oracle.tables(LINK_SEED, np.full(A, DELAY, np.int32), np.full(A, DROP), np.full(A, NOISE_P), None, DELAY,
                              int(extrapolate), Ts=Ts)


def oracle_loop(extrapolate, x_tol):
    """The closed loop of LOOP on the CPU oracle alone, plans on, under the link: (agent-cycles whose perceived solve
    converged, agent-cycles where both solves converged and the answer on the true tables is further than 100 x_tol
    from the one on the perceived tables, the smallest pair distance met, the largest departure of a table from its
    line)."""
    import plan12_oracle
    import sim12_oracle
    A, N, gait, seed, T, Ko, Kn = LOOP
    p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
    state, goal, obstacles, phase = head_on_team12(A, N, gait, seed)
    tab = loop_tables(A, extrapolate, p.Ts)
    st = link_oracle.new_state(A, N, tab["max_delay"])
    table, compared, matters, closest, err = None, 0, 0, np.inf, 0.0
    for c in range(T):
        b = sim12_oracle.cycle_inputs12(p, state, goal, obstacles, c, phase, gait)
        seen, seen_plan, _, st = link_oracle.update(c, 0, b["last_state"], table, tab, st)
        o, t = solve_seen(p, b, seen, seen_plan), solve_seen(p, b, b["last_state"], table)
        ok = converged(o["status"])
        compared += int(ok.sum())
        both = ok & converged(t["status"])
        matters += int((np.abs(o["x"][:, :12 * N] - t["x"][:, :12 * N]).max(1)[both] > 100 * x_tol).sum())
        err = max(err, o["line_err"], t["line_err"])
        P = b["last_state"][:, :2]
        closest = min(closest, (np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1)) + 1e9 * np.eye(A)).min())
        table = plan12_oracle.shift(plan12_oracle.plans_of(N, o["x"]))
        state = sim12_oracle.next_state12(o["x"])
    return compared, matters, float(closest), err
