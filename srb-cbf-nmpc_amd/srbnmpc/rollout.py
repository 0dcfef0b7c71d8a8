"""Closed-loop team rollout on the device (srb_sim_advance_device / srb_sim_metrics_device /
srb_rollout_device, include/srbnmpc.h): T control cycles of a whole agent batch with the nominal plant, the
goal-directed reference of workload.make_batch re-centred every cycle, and the team's safety log.

    r = Rollout(solver, goal, plans=True, obstacles=obstacles)
    r.reset(state)              # [A][4] x, xdot, y, ydot
    r.run(50)                   # the C driver: no host round trip inside
    out = r.results()           # traj, status, iters, min_d_agent, min_d_obs, fail_cycle, ...

step() is one cycle from Python (advance, [neighbour all-gather,] metrics, solve) and gives the same bits as
run(); shards of a team step in lockstep, each with its dist.NeighbourExchange.

With the solver's scene partition on (BatchSolver.set_scenes(team, n_obs); inputs from workload.make_scenes) the
batch is many independent teams rolled out by the same launches -- obstacles is then the scene-major table
[n_scenes * n_obs][2] -- and scene_results() reduces the metrics per scene.

With obs_vel ([n_obs][2], m/s) the obstacles move: every solve reads the velocities (srb_moving), and from the second
cycle on the table advances one cycle between the agents' advance and the metrics (srb_rollout_moving_device).  The
rollout then works on its own copy of `obstacles`; results()["obstacles"] is the current table.

With obs_eps ([n_obs], squared metres) every obstacle row has its own CBF level in the solve, with obs_clearance the
static columns are selected by clearance to the level set, and with obs_radius ([n_obs], m) d_obs is the clearance to
the obstacle bodies, min_i (dist_i - obs_radius[i]), and fail_cycle the first cycle with d_obs < 0 (srb_sizes,
srb_rollout_sized_device; srb12.Rollout12 likewise, srb12_rollout_sized_device).  The tables do not change over a
rollout.

With agent_rad / agent_pad ([n_all], m) every agent has its own safety radius towards its neighbours and its own pad on
the static obstacles' safety radii in the solve, with nbr_clearance the neighbour columns are selected by clearance
dist - agent_rad, and with agent_body ([n_all], m) d_agent is the clearance between bodies and collide_cycle the first
cycle with d_agent < 0 (srb_agent_sizes, srb_rollout_agents_device; srb12.Rollout12 likewise,
srb12_rollout_agents_device).  The tables do not change over a rollout and every shard holds them whole.

With kick_v / kick_p ([n_all], m/s and m), plant_hcom ([n_all], m) or pushes the plant is disturbed (srb_plant,
srb_sim_advance_plant_device / srb_rollout_plant_device; the SRB-12 mode's is Rollout12(plant=srb12.Plant12(...)),
srb12_plant): from the second cycle on the state that starts a cycle is the model's prediction -- or, with plant_hcom,
the roll of a LIP of that CoM height under the inputs the model applied -- plus a bounded uniform kick per cycle (Philox4x32-10 keyed by plant_seed, counter (cycle, global row)) and the
pushes due.  results()["disturbance"] logs what was added.  The tables do not change over a rollout and every shard
holds them whole; workload.plant_tables draws a set, workload.replicate_scenes tiles a scene for a Monte-Carlo over
the draws.

With link=srbnmpc.LinkModel(...) the neighbour link is degraded (srb_link, srb_link_update_device /
srb_rollout_link_device; srb12.Rollout12 likewise, srb12_rollout_link_device): every agent broadcasts its snapshot row and its shifted plan once per cycle, and
what the others hold of it is late by delay cycles, lost with probability drop and noisy by noise_p / noise_v at the
sender.  The solve and its selection read the perceived tables (Rollout.seen_state / seen_plan, readable after a step);
the metrics, traj and every log keep the truth.  results()["link_age"] logs the age of what was held.  The draws key on
(cycle, global row), so shards reproduce the team and the replicas of workload.replicate_scenes are a Monte-Carlo over
the link's draws as they are over the plant's; workload.link_tables draws a set of tables.

_RolloutBase is what this class and srb12.Rollout12 share: the checks of goal / phase / obstacles / obs_vel and of the
obstacle and agent size tables, the moving table's clone and its restore, the srb_moving, srb_sizes and
srb_agent_sizes of a call, the link's table checks, buffers and srb_link, the metrics call, the solve, metrics and log buffers, reset / advance / results /
scene_results and the preconditions of run().  A mode adds its state width, its own buffers, its srb_sim (_sim),
step() and the driver call of run() (_drive); the entry points are the solver's own (its _entry).
"""
from __future__ import annotations

import ctypes

from . import (AgentSizes, Batch, Link, LinkModel, Moving, Plant, Sim, Sizes, _check, _check_agent_array,
               _check_size_array, _check_vel_array, _dptr, _iptr, lib)

LINK_MAX_DELAY = 16                      # srb_link.max_delay's bound


def _check_tensor(t, shape, name, dtype, device):
    """Shape, dtype, contiguity (as _check_plan_array) and device of a tensor the library reads by pointer."""
    if not hasattr(t, "is_contiguous") or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                         f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    if t.device != device:
        raise ValueError(f"{name} must be on {device}, got {t.device}")


class _RolloutBase:
    """The closed loop of one mode's solver, as far as the LIP and the SRB-12 mode agree (the module docstring).
    Subclasses set the attributes below and define _sim(), step() and _drive()."""
    _nx = 4                              # state width: the rows of state, x0 and traj
    _name = "Rollout"                    # the class, in messages
    sharded = False                      # a shard of a larger team (Rollout only)

    def __init__(self, solver, goal, vref, phase, plans, log_x, obstacles, obs_vel, obs_horizon, obs_eps=None,
                 obs_radius=None, obs_clearance=False):
        import torch
        self.solver = solver
        p = solver.params
        if p.N < 4:
            raise ValueError(f"{self._name} needs N >= 4 (one cycle is one gait domain of 4 grids)")
        self.device = torch.device("cuda", solver.device)
        if not hasattr(goal, "shape") or len(goal.shape) != 2:
            raise ValueError("goal must be a [A][2] tensor")
        A = self.A = int(goal.shape[0])
        if A < 1 or A > solver.max_agents:
            raise ValueError(f"goal holds {A} agents, the solver takes 1 .. {solver.max_agents}")
        _check_tensor(goal, (A, 2), "goal", torch.float64, self.device)
        if phase is not None:
            _check_tensor(phase, (A,), "phase", torch.int32, self.device)
        if obstacles is not None:
            _check_tensor(obstacles, (obstacles.shape[0], 2), "obstacles", torch.float64, self.device)
            if obstacles.shape[0] == 0:
                obstacles = None
        if obs_vel is not None:
            if obstacles is None:
                raise ValueError("obs_vel needs obstacles (one velocity row per obstacle row)")
            _check_vel_array(obs_vel, obstacles.shape[0], torch.float64)
            if obs_vel.device != self.device:
                raise ValueError(f"obs_vel must be on {self.device}, got {obs_vel.device}")
            self.obstacles0 = obstacles
            obstacles = obstacles.clone()            # the rollout moves its table; the caller's stays
        elif obs_horizon:
            raise ValueError("obs_horizon needs obs_vel (the horizon-aware obstacle selection reads the velocities)")
        self.obs_vel, self.obs_horizon = obs_vel, bool(obs_horizon)
        for name, tab in (("obs_eps", obs_eps), ("obs_radius", obs_radius)):
            if tab is not None:
                if obstacles is None:
                    raise ValueError(f"{name} needs obstacles (one entry per obstacle row)")
                _check_size_array(tab, obstacles.shape[0], torch.float64, name, self.device)
        if obs_clearance and obs_eps is None:
            raise ValueError("obs_clearance needs obs_eps (the clearance selection reads the level table)")
        self.obs_eps, self.obs_radius, self.obs_clearance = obs_eps, obs_radius, bool(obs_clearance)
        self.sized = obs_eps is not None or obs_radius is not None     # run(): the _sized driver
        self.goal, self.phase, self.obstacles = goal, phase, obstacles
        self.vref, self.plans, self.log_x = float(vref), bool(plans), bool(log_x)
        N, nx = p.N, self._nx
        f8 = dict(dtype=torch.float64, device=self.device)
        i4 = dict(dtype=torch.int32, device=self.device)
        self.state, self.x0 = torch.zeros((A, nx), **f8), torch.zeros((A, nx), **f8)
        self.last_state = torch.zeros((A, 4), **f8)
        self.out = dict(x=torch.zeros((A, p.nv), **f8), obj=torch.zeros(A, **f8), status=torch.zeros((A, 2), **i4),
                        iters=torch.zeros((A, 2), **i4))
        self.plan_table = None
        if self.plans:
            self.plan_table = torch.zeros((A, N, 2), **f8)
            self.out["plan"] = torch.zeros((A, N, 2), **f8)
        self.metrics = dict(d_obs=torch.zeros(A, **f8), d_agent=torch.zeros(A, **f8), min_d_obs=torch.zeros(A, **f8),
                            min_d_agent=torch.zeros(A, **f8), fail_cycle=torch.full((A,), -1, **i4),
                            distance_to_fail=torch.zeros(A, **f8))
        self.cap = 0
        self.traj = self.status_log = self.iters_log = self.x_log = None
        self.c = 0
        self.flushed = True
        self._ready = False

    # ------------------------------------------------------------------ buffers
    def _reserve(self, cycles: int):
        """Log rows for `cycles` cycles (traj one more); grown by copying, so earlier rows stay."""
        import torch
        if cycles <= self.cap:
            return
        cap = max(cycles, 2 * self.cap, 8)
        A, nv = self.A, self.solver.params.nv

        def grow(old, rows, tail, dtype):
            new = torch.zeros((rows,) + tail, dtype=dtype, device=self.device)
            if old is not None:
                new[:old.shape[0]] = old
            return new
        self.traj = grow(self.traj, cap + 1, (A, self._nx), torch.float64)
        self.status_log = grow(self.status_log, cap, (A, 2), torch.int32)
        self.iters_log = grow(self.iters_log, cap, (A, 2), torch.int32)
        if self.log_x:
            self.x_log = grow(self.x_log, cap, (A, nv), torch.float64)
        if self.link is not None:
            self.age_log = grow(self.age_log, cap, (self._link_rows,), torch.int32)
        self.cap = cap

    def _moving(self) -> Moving:
        return Moving(_dptr(self.obs_vel), int(self.obs_horizon), _dptr(self.obstacles))

    def _sizes(self) -> Sizes:
        return Sizes(_dptr(self.obs_eps), _dptr(self.obs_radius), int(self.obs_clearance))

    agent_rad = agent_pad = agent_body = None     # the agent tables (_set_agent_sizes)
    nbr_clearance = agents = False

    def _set_agent_sizes(self, agent_rad, agent_pad, agent_body, nbr_clearance, n_all):
        """The agent tables of a rollout ([n_all] each, or None) after their checks, and with agent_body the
        collide_cycle buffer.  Called by the mode's __init__ once it knows n_all."""
        import torch
        for name, tab in (("agent_rad", agent_rad), ("agent_pad", agent_pad), ("agent_body", agent_body)):
            if tab is not None:
                _check_agent_array(tab, n_all, torch.float64, name, self.device, self.solver._agent_checked())
        if nbr_clearance and agent_rad is None:
            raise ValueError("nbr_clearance needs agent_rad (the clearance selection reads the radius table)")
        self.agent_rad, self.agent_pad, self.agent_body = agent_rad, agent_pad, agent_body
        self.nbr_clearance = bool(nbr_clearance)
        self.agents = agent_rad is not None or agent_pad is not None or agent_body is not None   # run(): the _agents driver
        if agent_body is not None:
            self.metrics["collide_cycle"] = torch.full((self.A,), -1, dtype=torch.int32, device=self.device)

    def _agent_sizes(self) -> AgentSizes:
        return AgentSizes(_dptr(self.agent_rad), _dptr(self.agent_pad), _dptr(self.agent_body), int(self.nbr_clearance),
                          _iptr(self.metrics.get("collide_cycle")))

    def _metrics(self, sim, stream):
        """The metrics of the current cycle on `sim` (the mode's srb_sim): with agent_body the agents entry point
        (obs_radius may be absent), with obs_radius alone the sized one."""
        s = self.solver
        if self.agent_body is not None:
            sz = ctypes.byref(self._sizes()) if self.obs_radius is not None else None
            _check(s._entry("sim_metrics_agents_device")(s._h, self.A, ctypes.byref(sim), sz,
                                                         ctypes.byref(self._agent_sizes()), self.c, s._stream(stream)))
        elif self.obs_radius is not None:
            _check(s._entry("sim_metrics_sized_device")(s._h, self.A, ctypes.byref(sim), ctypes.byref(self._sizes()),
                                                        self.c, s._stream(stream)))
        else:
            _check(s._entry("sim_metrics_device")(s._h, self.A, ctypes.byref(sim), self.c, s._stream(stream)))

    # ------------------------------------------------------------------ the degraded link (srb_link)
    link = seen_state = seen_plan = age_log = None     # the degraded link (_set_link)

    def _set_link(self, link, n_all):
        """The link's tables ([n_all] each, or None) after their checks, by name, and the link's own buffers.  Called
        by the mode's __init__ once it knows n_all."""
        import torch
        self.link = None
        self.seen_state = self.seen_plan = self.age_log = None
        if link is None:
            return
        if not isinstance(link, LinkModel):
            raise ValueError("link must be a srbnmpc.LinkModel (or None)")
        seed = int(link.seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError("link: seed must be 0 .. 2^64 - 1 (the 64-bit Philox key)")
        n = self._link_rows = int(n_all)
        if link.delay is not None:
            _check_tensor(link.delay, (n,), "link: delay", torch.int32, self.device)
            if bool((link.delay < 0).any()) or bool((link.delay > LINK_MAX_DELAY).any()):
                raise ValueError(f"link: delay must be 0 .. {LINK_MAX_DELAY} cycles")
        for name, tab in (("drop", link.drop), ("noise_p", link.noise_p), ("noise_v", link.noise_v)):
            if tab is None:
                continue
            _check_tensor(tab, (n,), f"link: {name}", torch.float64, self.device)
            if not bool(tab.isfinite().all()):
                raise ValueError(f"link: {name} must be finite")
            if bool((tab < 0).any()):
                raise ValueError(f"link: {name} must be >= 0")
            if name == "drop" and bool((tab > 1).any()):
                raise ValueError("link: drop must be <= 1 (a probability)")
        if not link.on:
            return                                   # nothing degrades: the plain rollout
        self.link = link
        self._link_seed, self._link_extrapolate = seed, int(bool(link.extrapolate))
        D = self._link_delay = 0 if link.delay is None else int(link.delay.max())
        N = self.solver.params.N
        f8 = dict(dtype=torch.float64, device=self.device)
        self._ring_state, self._held_state = torch.zeros((D + 1, n, 4), **f8), torch.zeros((n, 4), **f8)
        self._held_cycle = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.seen_state = torch.zeros((n, 4), **f8)
        self._ring_plan = self._held_plan = None
        if self.plans:
            self._ring_plan, self._held_plan = torch.zeros((D + 1, n, N, 2), **f8), torch.zeros((n, N, 2), **f8)
            self.seen_plan = torch.zeros((n, N, 2), **f8)

    def _link(self) -> Link:
        ln = self.link
        return Link(self._link_seed, _iptr(ln.delay), _dptr(ln.drop), _dptr(ln.noise_p), _dptr(ln.noise_v),
                    self._link_delay, self._link_extrapolate, _dptr(self._ring_state), _dptr(self._ring_plan),
                    _dptr(self._held_state), _dptr(self._held_plan), _iptr(self._held_cycle), _dptr(self.seen_state),
                    _dptr(self.seen_plan), _iptr(self.age_log))

    # ------------------------------------------------------------------ driving
    def reset(self, state):
        """Start state [A][4] (x, xdot, y, ydot; Rollout12: [A][12] p, roll/pitch/yaw, v, omega); the cycle count and
        the logs start over; with obs_vel the start table is restored.  Both are torch copies on torch's current
        stream: a caller who then passes another stream to step() / run() orders that stream after the current one
        first (nothing here does)."""
        import torch
        _check_tensor(state, (self.A, self._nx), "state", torch.float64, self.device)
        self.state.copy_(state)
        if self.obs_vel is not None:
            self.obstacles.copy_(self.obstacles0)    # the start table
        self.c = 0
        self.flushed = True
        self._ready = True

    def advance(self, stream=None):
        """The advance of the current cycle alone: state, x0, the reference, foot, last_state and the mode's other
        inputs of the solve (and the previous cycle's logs).  step() runs it itself; calling it first as well changes
        nothing (it rewrites the same values) and lets shards driven from one process fill their snapshot rows before
        a stand-in exchange gathers them."""
        if not self._ready:
            raise RuntimeError(f"{self._name}.advance before reset(state)")
        s = self.solver
        self._reserve(self.c + 1)
        _check(s._entry("sim_advance_device")(s._h, self.A, ctypes.byref(self._sim()), self.c, s._stream(stream)))

    def run(self, T: int, stream=None):
        """T cycles by the C driver (srb_rollout_device, srb12_rollout_device or, with plans / obs_vel, their
        variants), right after reset(): one call, nothing synchronises with the host inside.  A whole team only."""
        T = int(T)
        if not self._ready or self.c != 0:
            raise RuntimeError(f"{self._name}.run starts from reset(state) (use step() to go on)")
        if T < 0:
            raise ValueError("T must be >= 0")
        if self.sharded:
            raise ValueError("run() rolls out a whole team; a shard steps with its exchange (step)")
        sa = self.solver.scenes[0]
        if sa > 0 and self.A % sa != 0:
            raise ValueError(f"run() rolls out whole scenes: {self.A} agents are not a multiple of scene_agents = {sa}")
        self._reserve(T)
        self._drive(T, stream)
        self.c = T
        self.flushed = True

    def results(self, stream=None):
        """The logs and metrics so far, as tensors (views of this object's buffers; asynchronous like the
        launches -- synchronise before reading on the host): traj [T+1][A][nx] (nx 4, Rollout12: 12), status / iters
        [T][A][2], x [T][A][nv] (log_x), state [A][nx] (the end state), cycles, and d_obs, d_agent, min_d_obs,
        min_d_agent, fail_cycle, distance_to_fail [A] (with agent_body also collide_cycle [A]; with a link also link_age
        [T][n_all] int32: row c is, per global row, how many cycles before c the message the team holds of it was
        sent); with obs_vel, obstacles [n_obs][2] (the current table: the
        rows as the last cycle saw them)."""
        if not self._ready:
            raise RuntimeError(f"{self._name}.results before reset(state)")
        T = self.c
        self._reserve(max(T, 1))
        if not self.flushed:
            self.advance(stream)                 # the final advance: the last logs and the end state
            self.flushed = True
        elif T == 0:
            self.advance(stream)
        out = dict(cycles=T, traj=self.traj[:T + 1], status=self.status_log[:T], iters=self.iters_log[:T],
                   state=self.state, **self.metrics)
        if self.log_x:
            out["x"] = self.x_log[:T]
        if self.obs_vel is not None:
            out["obstacles"] = self.obstacles
        if self.link is not None:
            out["link_age"] = self.age_log[:T]
        return out

    def scene_results(self, stream=None):
        """results() reduced per scene of the solver's partition (set_scenes; a whole number of scenes), as device
        tensors [n_scenes]: min_d_agent and min_d_obs (the smallest over the scene's agents), n_failed (agents with
        fail_cycle >= 0) and n_not_converged (solves of the logged cycles that did not converge: QP stage neither
        OPTIMAL nor QP_WARM, or NLP stage not OPTIMAL), with agent_body n_collided (agents with collide_cycle >= 0); plus
        scene_agents and n_scenes.  Asynchronous like results()."""
        sa = self.solver.scenes[0]
        if sa <= 0:
            raise ValueError(f"scene_results needs the solver's scene partition ({type(self.solver).__name__}.set_scenes)")
        if self.sharded or self.A % sa != 0:
            raise ValueError(f"scene_results reduces whole scenes: {self.A} agents (a shard: {self.sharded}) "
                             f"are not a whole number of scenes of {sa}")
        return reduce_scenes(self.results(stream), sa)


class Rollout(_RolloutBase):
    """The closed loop of `solver` (a BatchSolver with N >= 4) for the agents whose goals are `goal` [A][2].

    vref      reference speed of the goal-directed line (workload.VREF)
    phase     [A] int32 or None: added to the cycle index for the trot parity
    plans     True: from the second cycle on, the inter-agent rows follow the neighbours' previous plans shifted
              by one gait domain (srb_batch.nbr_plan) instead of the constant-velocity guess
    log_x     True: keep every cycle's decision vectors (results()["x"], [T][A][nv])
    obstacles [n_obs][2] or None: the static obstacles, for the solve and for d_obs / fail_cycle
    obs_vel   [n_obs][2] or None: the obstacles' velocities (m/s).  The rollout then clones `obstacles` (it moves the
              table), reset() restores the start table, and every shard moves its own full copy (the same bits)
    obs_horizon  True: the static columns by closest predicted approach over the horizon (needs obs_vel)
    obs_eps   [n_obs] or None: the CBF level of each obstacle row, squared metres (None: eps_obs for every row)
    obs_radius  [n_obs] or None: the body radius (m) of each obstacle row: d_obs is then min_i (dist_i - obs_radius[i])
              and fail_cycle the first cycle with d_obs < 0 (None: centre distances and the 0.5 m test)
    obs_clearance  True: the static columns by clearance to the level set (needs obs_eps)
    agent_rad  [n_all] or None: the safety radius (m) of each agent: neighbour column j of agent g at the level
              (agent_rad[g] + agent_rad[sel[j]])^2 (None: eps_nbr for every pair)
    agent_pad  [n_all] or None: metres added to the safety radius of every static column of each agent
    agent_body  [n_all] or None: the body radius (m) of each agent: d_agent is then
              min_i (dist_i - (agent_body[g] + agent_body[i])), results() gains collide_cycle (the first cycle with
              d_agent < 0, else -1) and scene_results() n_collided (None: centre distances)
    nbr_clearance  True: the neighbour columns by clearance dist - agent_rad (needs agent_rad)
              The agent tables (srb_agent_sizes) are finite, agent_rad and agent_body not negative, and do not change
              over a rollout; every shard holds the whole tables.
    plant_seed  the key of the kicks' draws (0 .. 2^64 - 1); a rollout is reproducible per seed
    kick_v, kick_p  [n_all] or None: the bound (m/s, m) of the uniform kick every cycle adds to each agent's
              velocity / position (finite, not negative)
    plant_hcom  [n_all] or None: the CoM height (m, finite, positive) of each agent's plant; the state then follows
              the plant's own LIP under the model's inputs instead of the model's prediction (None: the prediction)
    pushes    None or (cycle int32 [P], agent int32 [P], dv float64 [P][2]), P <= 4096: entry p adds dv[p] (m/s) to the
              velocity of global row agent[p] at the start of cycle cycle[p] (>= 1: the first cycle starts from
              reset()'s state); entries on one agent and cycle add up in table order
              With any of these set advance(), step() and run() go through the plant entry points and results() gains
              disturbance [T][A][4] (dpx, dvx, dpy, dvy; row c - 1 is what the start of cycle c added).  Every shard
              holds the whole tables and draws by global row, so shards reproduce the team.
    link      None or a srbnmpc.LinkModel: the degraded neighbour link (seed, delay int32 [n_all] 0 .. 16, drop [n_all]
              0 .. 1, noise_p / noise_v [n_all] >= 0, extrapolate).  With any table set the solve and its selection read
              seen_state [n_all][4] / seen_plan [n_all][N][2] (attributes, readable after a step) instead of the
              gathered truth; the metrics and the logs keep the truth, and results() gains link_age [T][n_all] (cycles
              since the held message of each row was sent).  The rollout owns the link's ring, held and seen buffers,
              sized from max(delay), and reset() restarts the link.  Every shard holds the whole tables and computes
              the whole perceived table itself.  Not with the solver's plan_selection option (refused by name)
    agent_offset, n_all   a shard of a larger team: this batch is rows agent_offset .. agent_offset + A of the
              n_all-row neighbour table that step(exchange) gathers (default: the whole team)
    All tensors are float64 / int32, contiguous, on the solver's device.  Cycles count from 0 at reset()."""

    def __init__(self, solver, goal, vref: float = 0.27, phase=None, plans: bool = False, log_x: bool = False, *,
                 obstacles=None, agent_offset: int = 0, n_all: int | None = None, obs_vel=None, obs_horizon: bool = False,
                 obs_eps=None, obs_radius=None, obs_clearance: bool = False, agent_rad=None, agent_pad=None,
                 agent_body=None, nbr_clearance: bool = False, plant_seed: int = 0, kick_v=None, kick_p=None,
                 plant_hcom=None, pushes=None, link=None):
        import torch
        super().__init__(solver, goal, vref, phase, plans, log_x, obstacles, obs_vel, obs_horizon, obs_eps, obs_radius,
                         obs_clearance)
        A, p = self.A, solver.params
        self.agent_offset = int(agent_offset)
        self.n_all = A if n_all is None else int(n_all)
        if self.agent_offset < 0 or self.agent_offset + A > self.n_all:
            raise ValueError("agent_offset + A exceeds n_all")
        self._set_agent_sizes(agent_rad, agent_pad, agent_body, nbr_clearance, self.n_all)
        self._set_plant(plant_seed, kick_v, kick_p, plant_hcom, pushes)
        self._set_link(link, self.n_all)
        self.sharded = self.agent_offset != 0 or self.n_all != A
        f8 = dict(dtype=torch.float64, device=self.device)
        self.alpha_buf = torch.zeros((A, 4), **f8)
        self.ref = torch.zeros((A, 4 * p.N), **f8)
        self.foot = torch.zeros((A, p.N, 2, p.C), **f8)
        self.out["alpha"] = torch.zeros((A, 20), **f8)

    # ------------------------------------------------------------------ the disturbed plant (srb_plant)
    def _set_plant(self, seed, kick_v, kick_p, plant_hcom, pushes):
        """The plant tables ([n_all] each, or None) and the push table after their checks, by name."""
        import torch
        seed = int(seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError("plant_seed must be 0 .. 2^64 - 1 (the 64-bit Philox key)")
        for name, tab in (("kick_v", kick_v), ("kick_p", kick_p), ("plant_hcom", plant_hcom)):
            if tab is None:
                continue
            _check_size_array(tab, self.n_all, torch.float64, name, self.device)
            if not bool(tab.isfinite().all()):
                raise ValueError(f"{name} must be finite")
            if name == "plant_hcom" and bool((tab <= 0).any()):
                raise ValueError("plant_hcom must be > 0 (a CoM height in metres)")
            if name != "plant_hcom" and bool((tab < 0).any()):
                raise ValueError(f"{name} must be >= 0 (the bound of a uniform kick)")
        if pushes is not None:
            if not isinstance(pushes, (tuple, list)) or len(pushes) != 3:
                raise ValueError("pushes must be a triple (cycle int32 [P], agent int32 [P], dv float64 [P][2])")
            cyc, agent, dv = pushes
            P = int(cyc.shape[0]) if hasattr(cyc, "shape") and len(cyc.shape) == 1 else -1
            if P < 0 or P > 4096:
                raise ValueError("pushes: cycle must be an int32 tensor [P], P <= 4096")
            _check_tensor(cyc, (P,), "pushes: cycle", torch.int32, self.device)
            _check_tensor(agent, (P,), "pushes: agent", torch.int32, self.device)
            _check_tensor(dv, (P, 2), "pushes: dv", torch.float64, self.device)
            if P and (bool((agent < 0).any()) or bool((agent >= self.n_all).any())):
                raise ValueError(f"pushes: agent must be a global row 0 .. {self.n_all - 1}")
            pushes = (cyc, agent, dv) if P else None
        self.plant_seed, self.kick_v, self.kick_p, self.plant_hcom, self.pushes = seed, kick_v, kick_p, plant_hcom, pushes
        self.plant = kick_v is not None or kick_p is not None or plant_hcom is not None or pushes is not None
        self.dist_log = None
        self._advanced = -1             # the cycle whose advance has run (the plant's advance is not idempotent)

    def _plant(self) -> Plant:
        cyc, agent, dv = self.pushes if self.pushes is not None else (None, None, None)
        return Plant(self.plant_seed, _dptr(self.kick_v), _dptr(self.kick_p), _dptr(self.plant_hcom),
                     0 if cyc is None else cyc.shape[0], _iptr(cyc), _iptr(agent), _dptr(dv), _dptr(self.dist_log))

    def _reserve(self, cycles: int):
        super()._reserve(cycles)
        if self.plant and (self.dist_log is None or self.dist_log.shape[0] < self.cap):
            import torch
            new = torch.zeros((self.cap, self.A, 4), dtype=torch.float64, device=self.device)
            if self.dist_log is not None:
                new[:self.dist_log.shape[0]] = self.dist_log
            self.dist_log = new

    def reset(self, state):
        """As _RolloutBase.reset; the plant and the link start over (the link's first update, at cycle 0, is the
        complete exchange every row starts from: nothing of an earlier rollout is read)."""
        super().reset(state)
        self._advanced = -1

    def advance(self, stream=None):
        """As _RolloutBase.advance; with a disturbed plant through srb_sim_advance_plant_device, and once per cycle:
        the plant rolls on from the state of the previous cycle, so a second call for the same cycle is skipped
        (everything it would write is already there)."""
        if not self.plant:
            return super().advance(stream)
        if not self._ready:
            raise RuntimeError("Rollout.advance before reset(state)")
        if self._advanced == self.c:
            return
        s = self.solver
        self._reserve(self.c + 1)
        sim = self._sim()
        sim.n_all = self.n_all               # the rows of the plant tables (an advance reads no neighbour table)
        _check(lib().srb_sim_advance_plant_device(s._h, self.A, ctypes.byref(sim), ctypes.byref(self._plant()),
                                                  self.c, s._stream(stream)))
        self._advanced = self.c

    def results(self, stream=None):
        """As _RolloutBase.results; with a disturbed plant also disturbance [T][A][4]: row c - 1 is the (dpx, dvx, dpy,
        dvy) that the start of cycle c added to the plant's base state; with a link also link_age [T][n_all] int32: row c
        is, per global row, how many cycles before c the message the team holds of it was sent."""
        out = super().results(stream)
        if self.plant:
            out["disturbance"] = self.dist_log[:self.c]
        return out

    def _sim(self, nbr_state=None) -> Sim:
        nbr = self.last_state if nbr_state is None else nbr_state
        m, o = self.metrics, self.out
        return Sim(_dptr(self.state), _dptr(self.goal), _iptr(self.phase), self.vref, 0,
                   _dptr(o["x"]), _iptr(o["status"]), _iptr(o["iters"]),
                   _dptr(self.x0), _dptr(self.ref), _dptr(self.foot), _dptr(self.last_state), _dptr(self.alpha_buf),
                   _dptr(self.plan_table), _dptr(self.traj), _iptr(self.status_log), _iptr(self.iters_log),
                   _dptr(self.x_log), _dptr(self.obstacles), _dptr(nbr),
                   0 if self.obstacles is None else self.obstacles.shape[0], nbr.shape[0], self.agent_offset,
                   _dptr(m["d_obs"]), _dptr(m["d_agent"]), _dptr(m["min_d_obs"]), _dptr(m["min_d_agent"]),
                   _iptr(m["fail_cycle"]), _dptr(m["distance_to_fail"]))

    def step(self, exchange=None, plan_exchange=None, stream=None):
        """One cycle: advance, metrics, solve.  exchange (a dist.NeighbourExchange, or any callable
        [A][4] -> [n_all][4]): the all-gather of the snapshot rows between advance and metrics, for a shard;
        with plans, plan_exchange (a dist.PlanExchange) gathers the shifted plans likewise."""
        if not self._ready:
            raise RuntimeError("Rollout.step before reset(state)")
        if self.sharded and exchange is None:
            raise ValueError("a shard (agent_offset / n_all) steps with its neighbour exchange")
        if self.plans and exchange is not None and plan_exchange is None:
            raise ValueError("plans across shards need a plan_exchange (dist.PlanExchange)")
        s = self.solver
        self._reserve(self.c + 1)
        self.advance(stream)
        if self.obs_vel is not None and self.c > 0:          # the obstacles' cycle: every rank its own full copy
            s.advance_obstacles_device(self.obstacles, self.obs_vel, stream)
        nbr = self.last_state if exchange is None else exchange(self.last_state)
        import torch
        _check_tensor(nbr, (self.n_all, 4), "the exchanged neighbour table", torch.float64, self.device)
        self._metrics(self._sim(nbr), stream)
        table = None
        if self.plans and self.c > 0:
            table = self.plan_table if plan_exchange is None else plan_exchange(self.plan_table)
        if self.link is not None:                # the solve reads what is seen of the gathered truth
            if table is not None:
                _check_tensor(table, (self.n_all, s.params.N, 2), "the exchanged plan table", torch.float64, self.device)
            _check(lib().srb_link_update_device(s._h, self.n_all, ctypes.byref(self._link()), _dptr(nbr), _dptr(table),
                                                self.c, 0, s._stream(stream)))
            nbr = self.seen_state
            table = None if table is None else self.seen_plan
        s.solve_device(self.x0, self.ref, self.foot, self.obstacles, nbr, self.out, agent_offset=self.agent_offset,
                       stream=stream, alpha_buf=self.alpha_buf, nbr_plan=table, obs_vel=self.obs_vel,
                       obs_horizon=self.obs_horizon, obs_eps=self.obs_eps, obs_clearance=self.obs_clearance,
                       agent_rad=self.agent_rad, agent_pad=self.agent_pad, nbr_clearance=self.nbr_clearance)
        self.c += 1
        self.flushed = False

    def _drive(self, T: int, stream):
        s, o = self.solver, self.out
        b = Batch(None, None, None, _dptr(self.obstacles), None,
                  0 if self.obstacles is None else self.obstacles.shape[0], self.A, 0,
                  None, _dptr(o["x"]), _dptr(o["obj"]), _iptr(o["status"]), _iptr(o["iters"]),
                  None, _dptr(o["alpha"]), None, 0, None, _dptr(o.get("plan")))
        if self.link is not None:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            ag = ctypes.byref(self._agent_sizes()) if self.agents else None
            pl = ctypes.byref(self._plant()) if self.plant else None
            _check(lib().srb_rollout_link_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), mv, sz, ag, pl,
                                                 ctypes.byref(self._link()), T, s._stream(stream)))
            if self.plant:
                self._advanced = T
        elif self.plant:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            ag = ctypes.byref(self._agent_sizes()) if self.agents else None
            _check(lib().srb_rollout_plant_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), mv, sz, ag,
                                                  ctypes.byref(self._plant()), T, s._stream(stream)))
            self._advanced = T               # the driver's final advance was cycle T's
        elif self.agents:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            _check(lib().srb_rollout_agents_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), mv, sz,
                                                   ctypes.byref(self._agent_sizes()), T, s._stream(stream)))
        elif self.sized:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            _check(lib().srb_rollout_sized_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), mv,
                                                  ctypes.byref(self._sizes()), T, s._stream(stream)))
        elif self.obs_vel is not None:
            _check(lib().srb_rollout_moving_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()),
                                                   ctypes.byref(self._moving()), T, s._stream(stream)))
        else:
            _check(lib().srb_rollout_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), T,
                                            s._stream(stream)))


def reduce_scenes(res, scene_agents: int):
    """The per-scene reductions of Rollout.scene_results from a results() dict (torch tensors, any device):
    views [n_scenes][scene_agents] of the per-agent metrics, reduced along the scene."""
    sa = int(scene_agents)
    A = res["min_d_agent"].shape[0]
    if sa <= 0 or A % sa != 0:
        raise ValueError(f"{A} agents are not a whole number of scenes of {sa}")
    S = A // sa
    st = res["status"]                                       # [T][A][2]
    ok = ((st[..., 0] == 0) | (st[..., 0] == 4)) & (st[..., 1] == 0)
    out = dict(n_scenes=S, scene_agents=sa,
               min_d_agent=res["min_d_agent"].view(S, sa).amin(1), min_d_obs=res["min_d_obs"].view(S, sa).amin(1),
               n_failed=(res["fail_cycle"].view(S, sa) >= 0).sum(1),
               n_not_converged=(~ok).view(st.shape[0], S, sa).sum((0, 2)))
    if "collide_cycle" in res:                               # agent bodies (Rollout(agent_body=...))
        out["n_collided"] = (res["collide_cycle"].view(S, sa) >= 0).sum(1)
    return out
