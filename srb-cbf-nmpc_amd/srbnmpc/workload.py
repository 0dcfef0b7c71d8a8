"""Synthetic agent batches, deterministic per seed.

Distributions follow the reference's simulation setup where it has one:
  * start positions U[0,9] x U[-2,2]                     (src/A1_Sim.cpp:944-945)
  * obstacles U[0,9] x U[-2,2] + U[-0.6,0.6], clamped to [1,9] x [-3,3], 20 of them
                                                        (src/A1_Sim.cpp:946-980, NUMBER_OF_OBS)
  * reference: straight line to GOAL (10, 0) at 0.27 m/s (the speed of the logged
    instance, print_file.out), x, xdot, y, ydot per grid (copPlanner layout, MPC_dist.cpp:780)
  * footholds: default stance offsets (MPC_dist.cpp:1206-1209) around the CoM; trot pairs
    {FR,RL} / {FL,RR} alternating every gait domain of NDOMAIN = 4 grids (:906-916), so
    C = 2; C = 4 keeps all legs down (the reference's stand / first-domain case).
Deviation (documented in DESIGN.md): initial velocities are drawn toward the goal,
speed U[0, 0.3] plus U[-0.05, 0.05] per axis, instead of U[-0.3, 0.3] per axis -- with one
trot diagonal per domain the CoM-CoP rows (|p_k - u_{k+1}| <= mu h / sqrt 2) make a sideways
0.3 m/s start infeasible over a 0.43 s horizon, and the reference's QP has no slack on them.
Arenas scale with the batch so that agent density stays that of the reference's 4-agent
runs in a 9 m x 4 m field.
"""
from __future__ import annotations

import numpy as np

STANCE = np.array([[0.2188, 0.2188, -0.1472, -0.1472],     # x of FR, FL, RR, RL
                   [-0.1320, 0.1320, -0.1320, 0.1320]])    # y
TROT_PAIRS = ([0, 3], [1, 2])
GOAL = np.array([10.0, 0.0])
VREF = 0.27
TS = 43 * 0.001


def arena_scale(n_agents: int) -> float:
    return max(1.0, float(np.sqrt(n_agents / 4.0)))


def make_obstacles(rng, n_obs: int = 20, scale: float = 1.0):
    ox = rng.uniform(0, 9.0 * scale, n_obs)
    oy = rng.uniform(-2.0 * scale, 2.0 * scale, n_obs)
    ux = rng.uniform(-0.6, 0.6, n_obs)
    uy = rng.uniform(-0.6, 0.6, n_obs)
    rx = np.clip(ox + ux, 1.0, 9.0 * scale)
    ry = np.clip(oy + uy, -3.0 * scale, 3.0 * scale)
    return np.stack([rx, ry], 1)


def make_batch(n_agents: int, N: int = 10, C: int = 2, seed: int = 0, n_obs: int | None = None,
               velocity: str = "goal"):
    """Returns dict(x0 [A,4], ref [A,4N], foot [A,N,2,C], obstacles [n_obs,2],
    nbr_state [A,4] (x, y, xdot, ydot of every agent, the get_lastState layout)).
    velocity "goal" (default): initial velocities drawn toward the goal (the documented deviation);
    "free": U[-0.3, 0.3] per axis, uncorrelated with the goal and the trot support, which leaves
    some instances' CoM-CoP rows infeasible -- the hard workload of tests/test_gpu_parity.py
    (statuses other than OPTIMAL must agree with the oracle's too)."""
    rng = np.random.default_rng(seed)
    A = int(n_agents)
    sc = arena_scale(A)
    if n_obs is None:
        n_obs = int(round(20 * sc * sc))
    p0 = np.stack([rng.uniform(0, 9.0 * sc, A), rng.uniform(-2.0 * sc, 2.0 * sc, A)], 1)
    goal = GOAL * np.array([sc, 1.0]) + np.array([0.0, 0.0])
    d = goal - p0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v0 = d * rng.uniform(0, 0.3, (A, 1)) + rng.uniform(-0.05, 0.05, (A, 2))
    if velocity == "free":
        v0 = rng.uniform(-0.3, 0.3, (A, 2))
    x0 = np.stack([p0[:, 0], v0[:, 0], p0[:, 1], v0[:, 1]], 1)
    k = np.arange(N)
    ref = np.zeros((A, N, 4))
    ref[:, :, 0] = p0[:, None, 0] + d[:, None, 0] * VREF * TS * (k + 1)
    ref[:, :, 1] = d[:, None, 0] * VREF
    ref[:, :, 2] = p0[:, None, 1] + d[:, None, 1] * VREF * TS * (k + 1)
    ref[:, :, 3] = d[:, None, 1] * VREF
    foot = np.zeros((A, N, 2, C))
    phase = rng.integers(0, 4, A)
    for a in range(A):
        for kk in range(N):
            dom = (kk + phase[a]) // 4
            k_start = max(4 * dom - phase[a], 0)
            centre = p0[a] + d[a] * VREF * TS * k_start
            legs = TROT_PAIRS[dom % 2] if C == 2 else [0, 1, 2, 3]
            foot[a, kk] = STANCE[:, legs] + centre[:, None]
    obstacles = make_obstacles(rng, n_obs, sc)
    nbr_state = np.stack([x0[:, 0], x0[:, 2], x0[:, 1], x0[:, 3]], 1)
    return dict(x0=x0, ref=ref.reshape(A, 4 * N), foot=foot, obstacles=obstacles, nbr_state=nbr_state)


def obstacle_velocities(n_obs: int, seed: int, vmax: float = 1.0):
    """Velocities [n_obs][2] (m/s) for a moving obstacle table (BatchSolver.solve(obs_vel=...), Rollout(obs_vel=...)),
    deterministic per seed: speeds U[0.25 vmax, vmax] (all speeds are drawn first), headings U[0, 2 pi], from a
    generator of their own (100 + seed), so make_batch's draws for that seed stay as they are."""
    g = np.random.default_rng(100 + seed)
    sp = g.uniform(0.25 * vmax, vmax, n_obs)
    th = g.uniform(0, 2 * np.pi, n_obs)
    return np.stack([sp * np.cos(th), sp * np.sin(th)], 1)


EPS_OBS = float(np.float32(1.9))      # srb_params.eps_obs, (double)1.9f: the reference's one obstacle level
FAIL_RADIUS = 0.5                     # ... and its fail radius (updateDistance_to_fail)


def obstacle_sizes(n_obs: int, seed: int):
    """(eps, radius), each [n_obs], for a table of obstacles of different sizes (BatchSolver.solve(obs_eps=...),
    Rollout(obs_eps=..., obs_radius=...)), deterministic per seed: the CBF levels eps ~ U[0.6, 3.6] (squared metres)
    and the body radii 0.5 sqrt(eps / eps_obs), the reference's ratio of fail radius to safety radius.  From a
    generator of their own (200 + seed), so make_batch, make_scenes and obstacle_velocities draw what they drew."""
    eps = np.random.default_rng(200 + seed).uniform(0.6, 3.6, n_obs)
    return eps, FAIL_RADIUS * np.sqrt(eps / EPS_OBS)


EPS_NBR = float(np.float32(2.2))      # srb_params.eps_nbr, (double)2.2f: the reference's one inter-agent level


def agent_sizes(n_all: int, seed: int):
    """(rad, pad, body), each [n_all], for a team of agents of different sizes (BatchSolver.solve(agent_rad=...,
    agent_pad=...), Rollout(agent_rad=..., agent_pad=..., agent_body=...)), deterministic per seed: the safety radii
    rad ~ U[0.39, 0.94] m (pair levels (rad_a + rad_b)^2 between about 0.61 and 3.5, the range of obstacle_sizes),
    the pads rad - sqrt(eps_nbr) / 2 (what the agent's radius differs by from the reference's uniform one) and the
    body radii 0.5 rad / sqrt(eps_obs), the reference's ratio of fail radius to safety radius.  From a generator of
    their own (300 + seed), so every other draw of this module is what it was."""
    rad = np.random.default_rng(300 + seed).uniform(0.39, 0.94, n_all)
    return rad, rad - np.sqrt(EPS_NBR) / 2, FAIL_RADIUS * rad / np.sqrt(EPS_OBS)


SCENE_MAX_ATTEMPTS = 1000     # start draws per scene (make_scenes) before the clearance counts as impossible


def make_scenes(n_scenes: int, team: int, N: int = 10, C: int = 2, seed: int = 0, n_obs: int = 20,
                clearance: float = 0.5):
    """n_scenes independent teams of `team` agents for BatchSolver.set_scenes(team, n_obs), scene-major:
    dict(x0 [S*team,4], ref [S*team,4N], foot [S*team,N,2,C], obstacles [S*n_obs,2], nbr_state [S*team,4],
    goal [S*team,2], phase [S*team] int32).  Every scene is its own draw of the reference's arena at
    arena_scale(team) with make_batch's distributions, from a generator seeded by (seed, scene index) alone, so
    scene s is the same whatever n_scenes is.  A start closer than `clearance` to an obstacle of its scene or to an
    earlier start of its scene is drawn again (host-side rejection, deterministic); after SCENE_MAX_ATTEMPTS draws
    in one scene a ValueError names the scene."""
    S, A = int(n_scenes), int(team)
    if S < 1 or A < 1 or n_obs < 0:
        raise ValueError("make_scenes: n_scenes >= 1, team >= 1, n_obs >= 0")
    sc = arena_scale(A)
    goal1 = GOAL * np.array([sc, 1.0])
    k = np.arange(N)
    out = dict(x0=np.zeros((S * A, 4)), ref=np.zeros((S * A, N, 4)), foot=np.zeros((S * A, N, 2, C)),
               obstacles=np.zeros((S * n_obs, 2)), nbr_state=np.zeros((S * A, 4)), goal=np.tile(goal1, (S * A, 1)),
               phase=np.zeros(S * A, np.int32))
    for s in range(S):
        rng = np.random.default_rng([int(seed), s])
        obstacles = make_obstacles(rng, n_obs, sc)
        p0 = np.zeros((A, 2))
        attempts = 0
        for a in range(A):
            while True:
                if attempts >= SCENE_MAX_ATTEMPTS:
                    raise ValueError(f"make_scenes: scene {s}: no start {clearance} m clear of the scene's {n_obs} "
                                     f"obstacles and {a} earlier starts after {attempts} draws")
                attempts += 1
                q = np.array([rng.uniform(0, 9.0 * sc), rng.uniform(-2.0 * sc, 2.0 * sc)])
                taken = np.concatenate([obstacles, p0[:a]])
                if not taken.size or np.sqrt(((taken - q) ** 2).sum(1)).min() >= clearance:
                    break
            p0[a] = q
        d = goal1 - p0
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        v0 = d * rng.uniform(0, 0.3, (A, 1)) + rng.uniform(-0.05, 0.05, (A, 2))
        phase = rng.integers(0, 4, A)
        r = slice(s * A, (s + 1) * A)
        out["x0"][r] = np.stack([p0[:, 0], v0[:, 0], p0[:, 1], v0[:, 1]], 1)
        ref = out["ref"][r]
        ref[:, :, 0] = p0[:, None, 0] + d[:, None, 0] * VREF * TS * (k + 1)
        ref[:, :, 1] = d[:, None, 0] * VREF
        ref[:, :, 2] = p0[:, None, 1] + d[:, None, 1] * VREF * TS * (k + 1)
        ref[:, :, 3] = d[:, None, 1] * VREF
        for a in range(A):                                      # the trot schedule of make_batch
            for kk in range(N):
                dom = (kk + phase[a]) // 4
                k_start = max(4 * dom - phase[a], 0)
                centre = p0[a] + d[a] * VREF * TS * k_start
                legs = TROT_PAIRS[dom % 2] if C == 2 else [0, 1, 2, 3]
                out["foot"][s * A + a, kk] = STANCE[:, legs] + centre[:, None]
        out["obstacles"][s * n_obs:(s + 1) * n_obs] = obstacles
        out["nbr_state"][r] = np.stack([p0[:, 0], p0[:, 1], v0[:, 0], v0[:, 1]], 1)
        out["phase"][r] = phase
    out["ref"] = out["ref"].reshape(S * A, 4 * N)
    return out


HCOM = 0.29       # srb_params.hcom: the model's CoM height (MPC_dist.cpp:90-104)


def plant_tables(n_all: int, seed: int):
    """(kick_v, kick_p, plant_hcom), each [n_all], for a disturbed plant (Rollout(kick_v=..., kick_p=...,
    plant_hcom=...)), deterministic per seed.  kick_v ~ U[0.02, 0.08] m/s per cycle: 7 % to 30 % of the reference
    speed VREF = 0.27 m/s, velocity noise that is felt and that a walking robot still absorbs.  kick_p ~ U[0, 0.01] m
    per cycle: at most what VREF covers in one grid step (0.27 * 0.043 = 0.0116 m), a foot that slipped.  plant_hcom ~
    HCOM * U[0.85, 1.15] = 0.2465 .. 0.3335 m: a payload or a crouch the model does not know of, 15 % either way of
    the nominal 0.29 m.  From a generator of their own (400 + seed), so every other draw of this module is what it
    was."""
    g = np.random.default_rng(400 + seed)
    kick_v = g.uniform(0.02, 0.08, n_all)
    kick_p = g.uniform(0.0, 0.01, n_all)
    return kick_v, kick_p, HCOM * g.uniform(0.85, 1.15, n_all)


def link_tables(n_all: int, seed: int):
    """(delay int32, drop, noise_p, noise_v), each [n_all], for a degraded neighbour link
    (Rollout(link=srbnmpc.LinkModel(delay=..., drop=..., noise_p=..., noise_v=...))), deterministic per seed.  delay is
    0, 1 or 2 cycles, each equally likely: a snapshot up to 2 * 4 Ts = 0.344 s old (one control cycle is 4 Ts = 0.172 s),
    over which a neighbour at VREF = 0.27 m/s covers 0.093 m.  drop ~ U[0, 0.3]: up to three broadcasts in ten lost, a
    busy wireless channel.  noise_p ~ U[0, 0.03] m: up to 3 cm on each position component, about two thirds of what
    VREF covers in one cycle (0.27 * 0.172 = 0.046 m).  noise_v ~ U[0, 0.03] m/s: up to 11 % of VREF, which over the
    horizon of ten grids (0.43 s) misplaces the constant-velocity guess by 0.013 m.  From a generator of their own
    (600 + seed), so every other draw of this module is what it was."""
    g = np.random.default_rng(600 + seed)
    delay = g.integers(0, 3, n_all).astype(np.int32)
    drop = g.uniform(0.0, 0.3, n_all)
    noise_p = g.uniform(0.0, 0.03, n_all)
    return delay, drop, noise_p, g.uniform(0.0, 0.03, n_all)


def replicate_scenes(scenes: dict, copies: int):
    """A make_scenes (or make_scenes12) dict tiled `copies` times, scene-major: every array's rows repeated as a block, so rows
    [i * R, (i + 1) * R) of a table of R rows are replica i.  One scene (or set of scenes) then runs `copies` times in
    one launch with the same set_scenes(team, n_obs); under a disturbed plant each replica has draws of its own,
    because its global rows differ: the Monte-Carlo over disturbances that Rollout.scene_results() reduces.  The
    same holds under a degraded link (Rollout(link=...)): its loss and noise draws key on the global row too, so the
    replicas are a Monte-Carlo over the link's draws (tile the link's tables with np.tile likewise)."""
    copies = int(copies)
    if copies < 1:
        raise ValueError("replicate_scenes: copies >= 1")
    return {k: np.tile(np.asarray(v), (copies,) + (1,) * (np.asarray(v).ndim - 1)) for k, v in scenes.items()}


def cross_goals(goals, scene_agents: int, seed: int = 0):
    """Per-agent goals [n][2] exchanged within every scene of `scene_agents` rows: out[s * team + i] =
    goals[s * team + perm[i]] with perm one derangement (a permutation without a fixed point) of 0 .. team - 1, drawn
    from a generator of its own (700 + seed) and the same for every scene, so replicas of a scene
    (replicate_scenes) stay replicas.  Nobody keeps a goal, and nobody shares one: the rows of a scene must differ,
    or a ValueError names the scene.  make_scenes and make_scenes12 give a whole team ONE goal, which no exchange can
    tell apart; hand over the starts instead, scenes["nbr_state"][:, :2] of either, and every agent walks to where
    another one of its scene began, so that paths cross (the study DESIGN.md 10.14 asks for).  The input is not
    modified; the result goes to Rollout / Rollout12 as `goal`."""
    g = np.asarray(goals, dtype=np.float64)
    A = int(scene_agents)
    if g.ndim != 2 or g.shape[1] != 2:
        raise ValueError(f"cross_goals: goals must be [n][2], got {g.shape}")
    if A < 2 or g.shape[0] % A != 0:
        raise ValueError(f"cross_goals: {g.shape[0]} rows are not whole scenes of scene_agents = {A} >= 2 (a derangement "
                         "needs two)")
    rng = np.random.default_rng(700 + int(seed))
    while True:
        perm = rng.permutation(A)
        if not (perm == np.arange(A)).any():
            break
    sc = g.reshape(-1, A, 2)
    for s in range(sc.shape[0]):
        if len(np.unique(sc[s], axis=0)) != A:
            raise ValueError(f"cross_goals: scene {s} has two agents with one goal, so an exchange leaves them sharing it "
                             "(make_scenes gives a team one goal: hand over the starts, scenes['nbr_state'][:, :2])")
    return np.ascontiguousarray(sc[:, perm].reshape(-1, 2))


HCOM12 = 0.3      # SRB-12 mode: nominal CoM height of the synthetic batches


def make_batch12(n_agents: int, N: int = 10, gait: str = "trot", seed: int = 0, n_obs: int | None = None):
    """SRB-12 extension mode: the LIP batch's arena, starts, goal, obstacles
    and trot schedule, lifted to the 12-state single rigid body.  Returns dict(x0 [A,12],
    xref [A,N,12] (states x_1..x_N), foot [A,N,4,3] (world foot positions per grid),
    contact [A,N,4] int32, obstacles [n_obs,2], nbr_state [A,4] (x, y, xdot, ydot))."""
    rng = np.random.default_rng(seed)
    A = int(n_agents)
    sc = arena_scale(A)
    if n_obs is None:
        n_obs = int(round(20 * sc * sc))
    p0 = np.stack([rng.uniform(0, 9.0 * sc, A), rng.uniform(-2.0 * sc, 2.0 * sc, A)], 1)
    goal = GOAL * np.array([sc, 1.0])
    d = goal - p0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    head = np.arctan2(d[:, 1], d[:, 0])
    v0 = d * rng.uniform(0, 0.3, (A, 1)) + rng.uniform(-0.05, 0.05, (A, 2))
    x0 = np.zeros((A, 12))
    x0[:, 0:2] = p0
    x0[:, 2] = HCOM12 + rng.uniform(-0.01, 0.01, A)
    x0[:, 3:5] = rng.uniform(-0.02, 0.02, (A, 2))
    x0[:, 5] = head + rng.uniform(-0.1, 0.1, A)
    x0[:, 6:8] = v0
    x0[:, 9:12] = rng.uniform(-0.05, 0.05, (A, 3))
    k = np.arange(1, N + 1)
    xref = np.zeros((A, N, 12))
    xref[:, :, 0] = p0[:, None, 0] + d[:, None, 0] * VREF * TS * k
    xref[:, :, 1] = p0[:, None, 1] + d[:, None, 1] * VREF * TS * k
    xref[:, :, 2] = HCOM12
    xref[:, :, 5] = head[:, None]
    xref[:, :, 6] = d[:, None, 0] * VREF
    xref[:, :, 7] = d[:, None, 1] * VREF
    foot = np.zeros((A, N, 4, 3))
    contact = np.zeros((A, N, 4), np.int32)
    phase = rng.integers(0, 4, A)
    c, s = np.cos(head), np.sin(head)
    for a in range(A):
        Rm = np.array([[c[a], -s[a]], [s[a], c[a]]])
        off = (Rm @ STANCE).T                                   # (4, 2) stance offsets along the heading
        for kk in range(N):
            dom = (kk + phase[a]) // 4
            k_start = max(4 * dom - phase[a], 0)
            centre = p0[a] + d[a] * VREF * TS * k_start
            foot[a, kk, :, :2] = centre[None, :] + off
            legs = TROT_PAIRS[dom % 2] if gait == "trot" else [0, 1, 2, 3]
            contact[a, kk, legs] = 1
    obstacles = make_obstacles(rng, n_obs, sc)
    nbr_state = np.stack([x0[:, 0], x0[:, 1], x0[:, 6], x0[:, 7]], 1)
    return dict(x0=x0, xref=xref, foot=foot, contact=contact, obstacles=obstacles, nbr_state=nbr_state)


MASS12 = 12.453   # srb12_params.mass: the model's body mass (kg)


def plant_tables12(n_all: int, seed: int):
    """(kick_v, kick_p, kick_w, mass, inertia), each [n_all], for a disturbed plant of the SRB-12 mode
    (srb12.Plant12(kick_v=..., kick_p=..., kick_w=..., mass=..., inertia=...)), deterministic per seed.  kick_v ~
    U[0.02, 0.08] m/s and kick_p ~ U[0, 0.01] m per cycle: plant_tables' ranges for its reasons (7 % to 30 % of VREF; at
    most what VREF covers in one grid step).  kick_w ~ U[0.02, 0.1] rad/s per cycle, on each axis: from under half to
    twice the +-0.05 rad/s that make_batch12 draws for a start state's angular velocity, a body that is knocked and not
    tipped (0.1 rad/s held for a cycle of 0.172 s turns it by 1 degree).  mass ~ MASS12 * U[0.85, 1.15] = 10.6 ..
    14.3 kg: a payload the model does not know of, or a lighter battery, 15 % either way as plant_tables' CoM height.
    inertia ~ U[0.8, 1.25], a factor on the model's I_b: a payload away from the CoM changes the inertia by more than
    the mass, and the range is reciprocal so that lighter and heavier are equally likely in ratio.  From a generator of
    their own (500 + seed), so every other draw of this module is what it was."""
    g = np.random.default_rng(500 + seed)
    kick_v = g.uniform(0.02, 0.08, n_all)
    kick_p = g.uniform(0.0, 0.01, n_all)
    kick_w = g.uniform(0.02, 0.1, n_all)
    return kick_v, kick_p, kick_w, MASS12 * g.uniform(0.85, 1.15, n_all), g.uniform(0.8, 1.25, n_all)


def make_scenes12(n_scenes: int, team: int, N: int = 10, gait: str = "trot", seed: int = 0, n_obs: int = 20,
                  clearance: float = 0.5):
    """make_scenes lifted to the SRB-12 mode as make_batch12 lifts make_batch: n_scenes independent teams of `team`
    agents for Solver12.set_scenes(team, n_obs), scene-major: dict(x0 [S*team,12], xref [S*team,N,12],
    foot [S*team,N,4,3], contact [S*team,N,4] int32, obstacles [S*n_obs,2], nbr_state [S*team,4], goal [S*team,2],
    phase [S*team] int32).  Every scene is its own draw of the arena at arena_scale(team) from a generator seeded
    by (seed, scene index) alone, so scene s is the same whatever n_scenes is; starts keep `clearance` from the
    scene's obstacles and earlier starts by make_scenes' rejection rule (SCENE_MAX_ATTEMPTS draws a scene)."""
    S, A = int(n_scenes), int(team)
    if S < 1 or A < 1 or n_obs < 0:
        raise ValueError("make_scenes12: n_scenes >= 1, team >= 1, n_obs >= 0")
    sc = arena_scale(A)
    goal1 = GOAL * np.array([sc, 1.0])
    k = np.arange(1, N + 1)
    out = dict(x0=np.zeros((S * A, 12)), xref=np.zeros((S * A, N, 12)), foot=np.zeros((S * A, N, 4, 3)),
               contact=np.zeros((S * A, N, 4), np.int32), obstacles=np.zeros((S * n_obs, 2)),
               nbr_state=np.zeros((S * A, 4)), goal=np.tile(goal1, (S * A, 1)), phase=np.zeros(S * A, np.int32))
    for s in range(S):
        rng = np.random.default_rng([int(seed), s])
        obstacles = make_obstacles(rng, n_obs, sc)
        p0 = np.zeros((A, 2))
        attempts = 0
        for a in range(A):
            while True:
                if attempts >= SCENE_MAX_ATTEMPTS:
                    raise ValueError(f"make_scenes12: scene {s}: no start {clearance} m clear of the scene's {n_obs} "
                                     f"obstacles and {a} earlier starts after {attempts} draws")
                attempts += 1
                q = np.array([rng.uniform(0, 9.0 * sc), rng.uniform(-2.0 * sc, 2.0 * sc)])
                taken = np.concatenate([obstacles, p0[:a]])
                if not taken.size or np.sqrt(((taken - q) ** 2).sum(1)).min() >= clearance:
                    break
            p0[a] = q
        d = goal1 - p0
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        head = np.arctan2(d[:, 1], d[:, 0])
        v0 = d * rng.uniform(0, 0.3, (A, 1)) + rng.uniform(-0.05, 0.05, (A, 2))
        r = slice(s * A, (s + 1) * A)
        x0 = out["x0"][r]
        x0[:, 0:2] = p0
        x0[:, 2] = HCOM12 + rng.uniform(-0.01, 0.01, A)
        x0[:, 3:5] = rng.uniform(-0.02, 0.02, (A, 2))
        x0[:, 5] = head + rng.uniform(-0.1, 0.1, A)
        x0[:, 6:8] = v0
        x0[:, 9:12] = rng.uniform(-0.05, 0.05, (A, 3))
        xref = out["xref"][r]
        xref[:, :, 0] = p0[:, None, 0] + d[:, None, 0] * VREF * TS * k
        xref[:, :, 1] = p0[:, None, 1] + d[:, None, 1] * VREF * TS * k
        xref[:, :, 2] = HCOM12
        xref[:, :, 5] = head[:, None]
        xref[:, :, 6] = d[:, None, 0] * VREF
        xref[:, :, 7] = d[:, None, 1] * VREF
        phase = rng.integers(0, 4, A)
        cs, sn = np.cos(head), np.sin(head)
        for a in range(A):                                      # the trot schedule of make_batch12
            Rm = np.array([[cs[a], -sn[a]], [sn[a], cs[a]]])
            off = (Rm @ STANCE).T
            for kk in range(N):
                dom = (kk + phase[a]) // 4
                k_start = max(4 * dom - phase[a], 0)
                centre = p0[a] + d[a] * VREF * TS * k_start
                out["foot"][s * A + a, kk, :, :2] = centre[None, :] + off
                legs = TROT_PAIRS[dom % 2] if gait == "trot" else [0, 1, 2, 3]
                out["contact"][s * A + a, kk, legs] = 1
        out["obstacles"][s * n_obs:(s + 1) * n_obs] = obstacles
        out["nbr_state"][r] = np.stack([x0[:, 0], x0[:, 1], x0[:, 6], x0[:, 7]], 1)
        out["phase"][r] = phase
    return out
