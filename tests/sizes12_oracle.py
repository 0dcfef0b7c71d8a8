"""Reference answers for obstacle sizes in the SRB-12 mode (srb_sizes through srb12_*_sized*), from the oracle's own
pieces and numpy.

orc12_solve_agent knows two levels only, eps_obs for its static columns and eps_nbr for its neighbour columns, and it
selects for itself.  That is enough for a real answer to a level table that takes two values (e0, e1):

  solve_two_level   per agent, on a one-agent batch: the selected rows whose level is e0 are the oracle's obstacle table
                    (K_obs their count, eps_obs = e0), the rows at e1 a zero-velocity neighbour table (K_nbr their
                    count, eps_nbr = e1) with the agent's own row at agent_offset for the oracle to leave out
                    (moving12_oracle.solve_selected's device).  A zero-velocity neighbour row is predicted at
                    p + 0 * (Ts (k + 1)) = p, so both kinds of column are the same constraint at their own level.  The
                    oracle orders the columns its own way: a tolerance comparison.  With a velocity table every row
                    would have to go the neighbour way, so a moving world takes a one-level table or the certificate.
  rows_sized        any table, any K_nbr: plan12_oracle.rows / moving12_oracle.rows_moving with eps[:Ko] overwritten
                    by obs_eps[sel[:Ko]], for plan12_oracle.certificate.
  clearance_select  sizes_oracle.clearance_select on the rows the SRB-12 selection reads (plan12_oracle.lip_x0).
  two_level_table   the drawn table workload.obstacle_sizes(n_obs, seed) cut to LEVELS at CUT.

The metrics are sizes_oracle.Metrics on the com rows.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import moving12_oracle as mo
import oracle
import plan12_oracle as po
import sizes_oracle
from srbnmpc import workload

LEVELS = (1.2, 3.0)                  # the two levels (squared metres) ...
CUT = 2.1                            # ... of a drawn level below / at or above the cut


def two_level_table(n_obs, seed):
    """(eps, radius): workload.obstacle_sizes with every level cut to LEVELS; the radii are the drawn ones."""
    eps, radius = workload.obstacle_sizes(n_obs, seed)
    return np.where(eps < CUT, LEVELS[0], LEVELS[1]), radius


def solve_two_level(p, b, ob, obs_eps, sel, levels=LEVELS):
    """The batch b against the static rows sel [A][Ko] of ob [n_obs][2] whose levels obs_eps [n_obs] take the two
    values `levels` (p.K_nbr = 0).  Returns x, obj, status per agent."""
    ob = np.asarray(ob, np.float64).reshape(-1, 2)
    obs_eps = np.asarray(obs_eps, np.float64)
    e0, e1 = levels

    def one(a):
        rows = np.asarray(sel[a], np.int64)
        lv = obs_eps[rows]
        assert ((lv == e0) | (lv == e1)).all(), lv
        r0, r1 = rows[lv == e0], rows[lv == e1]
        q = oracle.params12(p.N, K_obs=len(r0), K_nbr=len(r1), eps_obs=e0, eps_nbr=e1)
        tab = None
        if len(r1):
            own = b["x0"][a][[0, 1, 6, 7]][None]
            tab = np.ascontiguousarray(np.concatenate([np.concatenate([ob[r1], np.zeros((len(r1), 2))], 1), own], 0))
        r = oracle.solve_batch12(q, b["x0"][a:a + 1], b["xref"][a:a + 1], b["foot"][a:a + 1], b["contact"][a:a + 1],
                                 np.ascontiguousarray(ob[r0]) if len(r0) else None, tab, agent_offset=len(r1), nthreads=1)
        return r["x"][0], r["status"][0], r["obj"][0]
    with ThreadPoolExecutor(8) as ex:                        # (the oracle call releases the interpreter lock)
        res = list(ex.map(one, range(b["x0"].shape[0])))
    return dict(x=np.array([r[0] for r in res]), status=np.array([r[1] for r in res], np.int32),
                obj=np.array([r[2] for r in res]))


def rows_sized(p, b, a, table, sel, obs_eps, ob=None, w=None):
    """obs [N][K][2], eps [K] of agent a for the device's sel with the gathered levels: the static columns at
    obs_eps[sel[j]] (a -1 column keeps eps_obs), moved when a velocity table w is given."""
    if w is None:
        obs, eps = po.rows(p, b, a, table, sel=sel)
    else:
        obs, eps = mo.rows_moving(p, b, a, table, sel, ob, w)
    eps = np.array(eps, copy=True)
    Ko = min(p.K_obs, np.asarray(b["obstacles"]).reshape(-1, 2).shape[0])
    for j in range(Ko):
        if sel[j] >= 0:
            eps[j] = np.asarray(obs_eps)[int(sel[j])]
    return obs, eps


def clearance_select(p, b, ob, obs_eps, Ko, vel=None, scene_agents=0, scene_obs=0):
    """sizes_oracle.clearance_select on the rows the SRB-12 selection reads; vel: over the horizon (p.N, p.Ts)."""
    x0 = np.array([po.lip_x0(x) for x in b["x0"]])
    return sizes_oracle.clearance_select(x0, ob, obs_eps, Ko, p.Ts, p.N, vel, scene_agents, scene_obs)


_refs = {}


def reference(shape):
    """For one of moving12_oracle.SHAPES0, computed once (read-only): moving12_oracle.reference's batch b, params p
    and unsized answer r0, the two-level table (eps, radius), the snapshot selection sel and the two-level answer r."""
    if shape not in _refs:
        N, Ko, A, gait, seed = shape
        R = mo.reference(shape)
        b, p = R["b"], R["p"]
        eps, radius = two_level_table(b["obstacles"].shape[0], seed)
        sel = mo.snapshot_select(b, b["obstacles"], Ko)
        r = solve_two_level(p, b, b["obstacles"], eps, sel)
        for v in list(r.values()) + [eps, radius, sel]:
            v.setflags(write=False)
        _refs[shape] = dict(b=b, p=p, r0=R["r0"], eps=eps, radius=radius, sel=sel, r=r)
    return _refs[shape]
