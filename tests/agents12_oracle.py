"""Reference answers for agent sizes in the SRB-12 mode (srb_agent_sizes through srb12_*_agents*), from the oracle's
own pieces and numpy.

orc12_solve_agent knows two levels only, eps_obs for its static columns and eps_nbr for its neighbour columns, and it
selects for itself.  That gives a real answer in four cases:

  (a) solve_uniform_pad   a uniform pad q: the oracle at eps_obs = (sqrt(e) + q)^2, the two rounded operations of the
                          kernel in numpy.
  (b) solve_uniform_rad   a uniform radius r: the oracle at eps_nbr = (r + r) * (r + r).
  (c) solve_pad_table     a per-agent pad table (and optionally a uniform radius): per agent, on a one-agent batch at
                          that agent's level, the whole tables and agent_offset = g so the oracle selects as the device.
  (d) solve_two_radii     a two-valued radius table (r0, r1) on a device with K_obs = 0, in a world where the rows of
                          radius r1 stand still (velocity 0 in nbr_state): per agent, on a one-agent batch, the selected
                          rows of radius r1 are the oracle's obstacle table at eps_obs = (rad[g] + r1)^2 (a zero-velocity
                          neighbour row is predicted at p + 0 * t = p, bit for bit the static row), the rows of radius
                          r0 its neighbour table at eps_nbr = (rad[g] + r0)^2 with the agent's own row at agent_offset
                          for the oracle to leave out (sizes12_oracle.solve_two_level's device).  The oracle orders the
                          columns its own way: a tolerance comparison.

Everything else goes through plan12_oracle.certificate on rows whose levels are agents_oracle.levels(...) (rows_agents),
the selection through agents_oracle.nbr_clear_select on the rows the SRB-12 selection reads (nbr_clear_select), the
metrics through agents_oracle.Metrics on the com rows.
"""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

import agents_oracle
import moving12_oracle as mo
import oracle
import plan12_oracle as po
from srbnmpc import workload

SHAPES12 = po.SHAPES12
# the K_obs = 0 forms of SHAPES12 (the device of (d)).  The N = 20 form draws its world from seed 48: in the world of
# seed 44 only two agents have a neighbour row that binds, whatever the radii, and tests/test_agents12.py asks for three
SHAPES_D = [(N, 0, Kn, A, gait, 48 if N == 20 else seed) for (N, Ko, Kn, A, gait, seed) in SHAPES12]
RADII = (0.45, 0.9)                  # (r0, r1) of (d): the scouts move, the carriers (r1) stand still
PAD_Q, RAD_R = 0.3, 0.6              # the uniform pad of (a), the uniform radius of (b)


def pad_table(A, seed):
    """The per-agent pads of (c): U[0.1, 0.6] m from a generator of its own.  (workload.agent_sizes' pads,
    rad - sqrt(eps_nbr) / 2, are mostly negative and leave the (4, 1, 2, 8) shape with one agent that moves.)"""
    return np.random.default_rng(700 + seed).uniform(0.1, 0.6, A)


def pad_level(e, q):
    """(sqrt(e) + q)^2, one rounded operation each."""
    t = np.sqrt(np.float64(e)) + np.float64(q)
    return float(t * t)


def pair_level(ra, rb):
    """(ra + rb)^2, one rounded add and one rounded multiply."""
    s = np.float64(ra) + np.float64(rb)
    return float(s * s)


def params(p, **kw):
    """oracle.params12 with p's N, K_obs, K_nbr and the levels given."""
    kw = dict(dict(K_obs=p.K_obs, K_nbr=p.K_nbr, eps_obs=p.eps_obs, eps_nbr=p.eps_nbr), **kw)
    return oracle.params12(p.N, **kw)


def _solve(q, b, nbr):
    return oracle.solve_batch12(q, b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], nbr)


def solve_uniform_pad(p, b, q):
    """(a): every agent's pad is q."""
    return _solve(params(p, eps_obs=pad_level(p.eps_obs, q)), b, b["nbr_state"] if p.K_nbr > 0 else None)


def solve_uniform_rad(p, b, r):
    """(b): every agent's radius is r."""
    return _solve(params(p, eps_nbr=pair_level(r, r)), b, b["nbr_state"])


def _per_agent(one, A):
    with ThreadPoolExecutor(8) as ex:                        # (the oracle call releases the interpreter lock)
        res = list(ex.map(one, range(A)))
    return dict(x=np.array([r["x"][0] for r in res]), status=np.array([r["status"][0] for r in res], np.int32),
                obj=np.array([r["obj"][0] for r in res]), iters=np.array([r["iters"][0] for r in res], np.int32))


def solve_pad_table(p, b, pad, rad=None, agent_offset=0):
    """(c): agent a (table row agent_offset + a) at eps_obs = (sqrt(eps_obs) + pad[g])^2; rad: a uniform radius r on
    top (eps_nbr = (r + r)^2), or None."""
    nbr = b["nbr_state"] if p.K_nbr > 0 else None
    en = p.eps_nbr if rad is None else pair_level(rad, rad)

    def one(a):
        g = agent_offset + a
        q = params(p, eps_obs=pad_level(p.eps_obs, pad[g]), eps_nbr=en)
        return oracle.solve_batch12(q, b["x0"][a:a + 1], b["xref"][a:a + 1], b["foot"][a:a + 1], b["contact"][a:a + 1],
                                    b["obstacles"], nbr, agent_offset=g, nthreads=1)
    return _per_agent(one, b["x0"].shape[0])


def two_radii_world(shape):
    """For one of SHAPES_D: (b, rad).  rad takes RADII[1] where workload.agent_sizes draws a radius at or above the
    median, else RADII[0]; the batch is plan12_oracle's with the velocity of every RADII[1] row of nbr_state zeroed."""
    N, Ko, Kn, A, gait, seed = shape
    b = dict(workload.make_batch12(A, N, gait, seed=seed))
    drawn, _, _ = workload.agent_sizes(A, seed)
    rad = np.where(drawn >= np.median(drawn), RADII[1], RADII[0])
    nbr = np.array(b["nbr_state"], dtype=np.float64)
    nbr[rad == RADII[1], 2:] = 0.0
    b["nbr_state"] = np.ascontiguousarray(nbr)
    return b, rad


def snapshot_nbr(p, b, a, g=None):
    """The neighbour columns of agent a by the snapshot selection, clamped to the other rows as the C ABI clamps them."""
    idx = po.select(p, b, a, g)
    kn = min(p.K_nbr, b["nbr_state"].shape[0] - 1)
    return np.asarray(idx[p.K_obs:p.K_obs + kn], np.int32)


def solve_two_radii(p, b, rad, sel, radii=RADII):
    """(d): the batch b (p.K_obs = 0) against the neighbour rows sel [A][Kn] of b["nbr_state"], whose radii rad [n_all]
    take the two values `radii` and whose rows of radius radii[1] have velocity 0."""
    nbr = np.asarray(b["nbr_state"], np.float64)
    r0, r1 = radii
    assert (nbr[rad == r1, 2:] == 0.0).all()

    def one(a):
        rows = np.asarray(sel[a], np.int64)
        rows = rows[rows >= 0]
        rr = rad[rows]
        assert ((rr == r0) | (rr == r1)).all(), rr
        still, moving = rows[rr == r1], rows[rr == r0]
        q = oracle.params12(p.N, K_obs=len(still), K_nbr=len(moving), eps_obs=pair_level(rad[a], r1),
                            eps_nbr=pair_level(rad[a], r0))
        tab = None
        if len(moving):
            own = b["x0"][a][[0, 1, 6, 7]][None]
            tab = np.ascontiguousarray(np.concatenate([nbr[moving], own], 0))
        return oracle.solve_batch12(q, b["x0"][a:a + 1], b["xref"][a:a + 1], b["foot"][a:a + 1], b["contact"][a:a + 1],
                                    np.ascontiguousarray(nbr[still, :2]) if len(still) else None, tab,
                                    agent_offset=len(moving), nthreads=1)
    return _per_agent(one, b["x0"].shape[0])


def levels12(p, Ko, sel, g, rad=None, pad=None, obs_eps=None):
    """eps [K] of the device's columns sel (Ko static, then the neighbour columns): eps_obs / eps_nbr, the obs_eps
    gather, then agents_oracle.levels (rad, then pad)."""
    sel = np.asarray(sel)
    k = SimpleNamespace(K_obs=Ko, K_nbr=len(sel) - Ko)
    eps = np.array([p.eps_obs] * k.K_obs + [p.eps_nbr] * k.K_nbr)
    if obs_eps is not None:
        for j in range(Ko):
            if sel[j] >= 0:
                eps[j] = np.asarray(obs_eps)[int(sel[j])]
    return agents_oracle.levels(k, eps, sel, g, rad, pad)


def rows_agents(p, b, a, table, sel, rad=None, pad=None, obs_eps=None, ob=None, w=None, g=None):
    """obs [N][K][2], eps [K] of agent a (table row g, default a) for the device's sel: sizes12_oracle.rows_sized's
    rows with the levels of levels12."""
    if w is None:
        obs, _ = po.rows(p, b, a, table, sel=sel)
    else:
        obs, _ = mo.rows_moving(p, b, a, table, sel, ob, w)
    Ko = min(p.K_obs, np.asarray(b["obstacles"]).reshape(-1, 2).shape[0])
    return obs, levels12(p, Ko, sel, a if g is None else g, rad, pad, obs_eps)


def nbr_clear_select(b, rad, K, plan=None, lo=0, scene_agents=0):
    """agents_oracle.nbr_clear_select on the rows the SRB-12 selection reads (plan12_oracle.lip_x0)."""
    x0 = np.array([po.lip_x0(x) for x in b["x0"]])
    return agents_oracle.nbr_clear_select(x0, b["nbr_state"], rad, K, plan, lo, scene_agents)


_refs = {}


def reference(shape, what):
    """Computed once (read-only).  For one of SHAPES12: "none" the oracle's answer without a table, "pad" (a), "rad"
    (b), "pad_table" (c) with pad_table's pads; for one of SHAPES_D: "two" dict(b, rad, sel, r, r0) of (d),
    r0 the answer at eps_nbr for every pair."""
    key = (shape, what)
    if key not in _refs:
        N, Ko, Kn, A, gait, seed = shape
        p = oracle.params12(N, K_obs=Ko, K_nbr=Kn)
        if what == "two":
            b, rad = two_radii_world(shape)
            sel = np.array([snapshot_nbr(p, b, a) for a in range(A)], np.int32)
            r = dict(b=b, rad=rad, sel=sel, p=p, r=solve_two_radii(p, b, rad, sel), r0=_solve(p, b, b["nbr_state"]))
        else:
            b = po.reference(shape)["b"]
            if what == "none":
                r = po.reference(shape)["r_cv"]
            elif what == "pad":
                r = solve_uniform_pad(p, b, PAD_Q)
            elif what == "rad":
                r = solve_uniform_rad(p, b, RAD_R)
            else:
                r = solve_pad_table(p, b, pad_table(A, seed))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            elif isinstance(v, dict):
                for u in v.values():
                    if isinstance(u, np.ndarray):
                        u.setflags(write=False)
        _refs[key] = r
    return _refs[key]
