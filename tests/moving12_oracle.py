"""Reference answers for SRB-12 solves against moving obstacles (srb_moving through srb12_*_moving*), from the
oracle's own pieces and numpy.

orc12_solve_agent takes no per-grid rows, but its neighbour rows are already p + v * (Ts (k + 1)), one rounded
multiply and one rounded add, with a settable eps.  So a moving obstacle table (ob, w) is handed to it as a
neighbour table:

  solve_moving      K_nbr = 0, snapshot selection.  The device's answer for K_obs = Ko and the table (ob, w) must
                    equal oracle.solve_batch12 with K_obs = 0, K_nbr = Ko, eps_nbr = eps_obs, the neighbour table
                    concat(ob, w) and agent_offset = n_obs (past the table: no row is left out as "self").  With
                    w = 0 this is the static oracle bit for bit, provided every obstacle is within 1000 m and
                    Ko <= n_obs - 1 (the oracle clamps K_nbr to n_all - 1; tests/test_moving12.py pins both).
  solve_selected    the same call per agent, on a one-agent batch whose table holds only that agent's selected rows
                    and, at agent_offset, the agent's own row (the oracle clamps K_nbr to the rows other than "self",
                    so without it the farthest selected row would be dropped); the oracle then picks all of them, in
                    its own order: a tolerance comparison.
  rows_moving       K_nbr > 0: no oracle answers it; plan12_oracle.rows with the static columns overwritten by
                    ob[sel[j]] + w[sel[j]] * (Ts (k + 1)), for plan12_oracle.certificate.
  closed_loop12_moving   the oracle-only closed loop in the moving world, on sim12_oracle's advance, sim_oracle's
                    Metrics on the moved table and moving_oracle.advance_obstacles.
"""
import numpy as np

import moving_oracle
import oracle
import plan12_oracle
import sim12_oracle
import sim_oracle
from srbnmpc import workload

# the K_nbr = 0 forms of plan12_oracle.SHAPES12 (the two (10, 3, 8, 16, ..) shapes share one): (N, K_obs, A, gait, seed)
SHAPES0 = [(10, 3, 16, "trot", 41), (4, 1, 8, "trot", 45), (6, 2, 12, "stand", 45), (20, 3, 8, "trot", 44)]
# the closed-loop runs, sim12_oracle.RUNS12's layout (A, N, gait, seed, T, K_obs, K_nbr), vmax 1.0
RUNS0 = [(8, 6, "stand", 7, 6, 1, 0), (8, 10, "trot", 6, 6, 3, 0), (8, 4, "trot", 6, 8, 1, 0), (6, 20, "trot", 8, 4, 3, 0)]


def as_nbr_params(p):
    """The oracle parameters that read p's static columns as neighbour columns."""
    return oracle.params12(p.N, K_obs=0, K_nbr=p.K_obs, eps_nbr=p.eps_obs)


def solve_moving(p, b, ob, w):
    """Reference 1 (p.K_nbr = 0): the batch b against the obstacles ob [n_obs][2] moving at w [n_obs][2]."""
    ob = np.asarray(ob, np.float64).reshape(-1, 2)
    tab = np.ascontiguousarray(np.concatenate([ob, np.asarray(w, np.float64).reshape(-1, 2)], 1))
    return oracle.solve_batch12(as_nbr_params(p), b["x0"], b["xref"], b["foot"], b["contact"], None, tab,
                                agent_offset=ob.shape[0])


def solve_selected(p, b, ob, w, sel):
    """Reference 2 (p.K_nbr = 0): per agent, the rows sel[a] alone as the table.  Returns x, status [A].."""
    ob, w = np.asarray(ob, np.float64).reshape(-1, 2), np.asarray(w, np.float64).reshape(-1, 2)
    q = as_nbr_params(p)
    xs, st = [], []
    for a in range(b["x0"].shape[0]):
        rows = np.asarray(sel[a], np.int64)
        # (the oracle clamps K_nbr to n_all - 1, the rows other than "self": one more row, the agent's own, stands at
        # index agent_offset for it to leave out)
        own = b["x0"][a][[0, 1, 6, 7]][None]
        tab = np.ascontiguousarray(np.concatenate([np.concatenate([ob[rows], w[rows]], 1), own], 0))
        r = oracle.solve_batch12(q, b["x0"][a:a + 1], b["xref"][a:a + 1], b["foot"][a:a + 1], b["contact"][a:a + 1], None,
                                 tab, agent_offset=len(rows), nthreads=1)
        xs.append(r["x"][0]); st.append(r["status"][0])
    return dict(x=np.array(xs), status=np.array(st, np.int32))


def snapshot_select(b, ob, Ko):
    """[A][min(Ko, n_obs)]: the rows nearest now, the snapshot selection of the static columns."""
    x0 = np.array([plan12_oracle.lip_x0(x) for x in b["x0"]])
    return moving_oracle.select_by_key(moving_oracle.snapshot_keys(x0, ob), Ko)


def horizon_select(p, b, ob, w, Ko, scene_agents=0, scene_obs=0):
    """moving_oracle.horizon_select on the rows the SRB-12 selection reads."""
    x0 = np.array([plan12_oracle.lip_x0(x) for x in b["x0"]])
    return moving_oracle.horizon_select(p.Ts, p.N, x0, ob, w, Ko, scene_agents, scene_obs)


def rows_moving(p, b, a, table, sel, ob, w):
    """Reference 3: obs [N][K][2], eps [K] of agent a for the device's sel, the static columns moved."""
    obs, eps = plan12_oracle.rows(p, b, a, table, sel=sel)
    ob, w = np.asarray(ob, np.float64).reshape(-1, 2), np.asarray(w, np.float64).reshape(-1, 2)
    Ko = min(p.K_obs, ob.shape[0])
    for j in range(Ko):
        i = int(sel[j])
        if i >= 0:
            for k in range(p.N):
                obs[k, j] = ob[i] + w[i] * (p.Ts * (k + 1))
    return obs, eps


def world12(run, vmax=1.0):
    """sim12_oracle.team12 of a run plus the obstacles' velocities."""
    A, N, gait, seed, T, Ko, Kn = run
    state, goal, ob, phase = sim12_oracle.team12(A, N, gait, seed)
    return state, goal, ob, phase, workload.obstacle_velocities(ob.shape[0], seed, vmax)


_loops = {}


def closed_loop12_moving(run, aware=True, vmax=1.0):
    """Reference 4 (K_nbr = 0), computed once (read-only): per cycle the agents' advance, for c > 0 the obstacles'
    advance, the metrics on the moved table, the solve -- aware of the velocities, or (aware=False) the same moving
    world solved as if the table it re-reads every cycle were static.  dict(p, traj [T+1][A][12], status [T][A][2],
    x [T][A][24N+1], obstacles (the last cycle's table), metrics)."""
    key = (run, aware, vmax)
    if key not in _loops:
        A, N, gait, seed, T, Ko, Kn = run
        assert Kn == 0
        p = oracle.params12(N, K_obs=Ko, K_nbr=0)
        st, goal, ob, phase, w = world12(run, vmax)
        traj, status, xs = [st], [], []
        m = sim_oracle.Metrics(0)
        for c in range(T):
            if c > 0:
                ob = moving_oracle.advance_obstacles(p.Ts, ob, w)
            b = sim12_oracle.cycle_inputs12(p, st, goal, ob, c, phase, gait)
            m.update(c, b["com"], ob, b["nbr_state"])
            r = solve_moving(p, b, ob, w if aware else np.zeros_like(w))
            status.append(r["status"]); xs.append(r["x"])
            st = sim12_oracle.next_state12(r["x"])
            traj.append(st)
        out = dict(p=p, traj=np.array(traj), status=np.array(status), x=np.array(xs), obstacles=ob,
                   metrics=m.as_dict())
        for v in list(out.values()) + list(out["metrics"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _loops[key] = out
    return _loops[key]


_refs = {}


def reference(shape, vmax=1.0):
    """For one of SHAPES0, computed once (read-only): the batch b, the oracle params p (K_nbr = 0), the velocities w,
    the static oracle answer r0 and the moving answer r of solve_moving."""
    if (shape, vmax) not in _refs:
        N, Ko, A, gait, seed = shape
        b = workload.make_batch12(A, N, gait, seed=seed)
        p = oracle.params12(N, K_obs=Ko, K_nbr=0)
        w = workload.obstacle_velocities(b["obstacles"].shape[0], seed, vmax)
        r0 = oracle.solve_batch12(p, b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], None)
        r = solve_moving(p, b, b["obstacles"], w)
        for d in (r0, r):
            for v in d.values():
                v.setflags(write=False)
        w.setflags(write=False)
        _refs[(shape, vmax)] = dict(b=b, p=p, w=w, r0=r0, r=r)
    return _refs[(shape, vmax)]
