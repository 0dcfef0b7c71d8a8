"""SRB-12 extension mode: the north star's 12-state single-rigid-body CBF-NMPC on the GPU
(srb12_* in include/srbnmpc.h, csrc/srb12_kernels.hip).

The reference declares this solver (FastMPC::runMPC / MPC_Cost / MPC_Constraints /
getLinearDynamics, /root/reference/include/fast_MPC.hpp:98-103) without a body, so there is no
reference call surface to mirror: Solver12 follows BatchSolver's shape (host numpy solve, device
torch solve on a stream).  Problem statement: DESIGN.md section 11; checker: oracle/srb12.c.

Team features, as the LIP mode's: Solver12.set_scenes partitions a batch into independent teams
(srb12_ctx_set_scenes; inputs from workload.make_scenes12), and Rollout12 is the closed-loop rollout on the
device (csrc/srb12_sim.hip, srb12_rollout_device; DESIGN.md sections 9 and 10.4).  Neighbour plans (Plans12,
srb12_plans): Solver12.solve / solve_device take nbr_plan and return plan, Solver12.solve_coupled_device is the
Jacobi driver over the plans, and Rollout12(plans=True) feeds last cycle's plans forward.  Moving
obstacles (srb_moving): obs_vel / obs_horizon on Solver12.solve, solve_device, solve_coupled_device
and Rollout12, Solver12.advance_obstacles_device; velocities from workload.obstacle_velocities.  Obstacle sizes
(srb_sizes): obs_eps / obs_clearance on the same three solver calls, obs_eps / obs_radius /
obs_clearance on Rollout12; tables from workload.obstacle_sizes.  Agent sizes (srb_agent_sizes):
agent_rad / agent_pad / nbr_clearance on the same three solver calls, those and agent_body on Rollout12; tables from
workload.agent_sizes.  Degraded neighbour link (srb_link): Rollout12(link=srbnmpc.LinkModel(...)),
Solver12.solve_device(own_plan=); tables from workload.link_tables.

The host layer of these features is written once for both modes: Solver12 is a _SolverBase (srbnmpc/__init__.py: the
context's life, _stream, set_scenes, the Jacobi loop), Rollout12 a rollout._RolloutBase (the checks, buffers, logs,
reset / advance / run / results, the obstacle and agent size tables' checks and the metrics call), and the pointer
casts, the (Ko, Kn) clamp and the srb_moving / srb_sizes / srb_agent_sizes checks are the package's.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import (AgentSizes, Link, Moving, Sizes, _SolverBase, _agent_args, _check, _check_plan_array, _check_vel_array,
               _clamp_selected, _dp, _dptr, _ip, _iptr, _moving_args, _p, _sizes_args, lib, workload)
from .rollout import _RolloutBase

_p12_fields = [("N", ctypes.c_int), ("K_obs", ctypes.c_int), ("K_nbr", ctypes.c_int),
               ("Ts", ctypes.c_double), ("mass", ctypes.c_double), ("Ib", ctypes.c_double * 9),
               ("grav", ctypes.c_double), ("mu", ctypes.c_double), ("fmax", ctypes.c_double),
               ("q", ctypes.c_double * 12), ("qN", ctypes.c_double * 12), ("r", ctypes.c_double * 3),
               ("Sw", ctypes.c_double), ("eps_obs", ctypes.c_double), ("eps_nbr", ctypes.c_double),
               ("tol", ctypes.c_double), ("qp_maxit", ctypes.c_int), ("nlp_maxit", ctypes.c_int),
               ("use_nlp", ctypes.c_int), ("z0", ctypes.c_double),
               ("tol_final", ctypes.c_double), ("polish", ctypes.c_int), ("tol_qp", ctypes.c_double)]


class Params12(ctypes.Structure):
    """Mirror of srb12_params (the oracle's orc12_params has the same layout)."""
    _fields_ = _p12_fields

    @property
    def nv(self) -> int:
        return 24 * self.N + 1


class Batch12(ctypes.Structure):
    """Mirror of srb12_batch (struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("x0", _dp), ("xref", _dp), ("foot", _dp), ("contact", _ip),
                ("obstacles", _dp), ("nbr_state", _dp), ("n_obs", ctypes.c_int), ("n_all", ctypes.c_int),
                ("agent_offset", ctypes.c_int), ("x_qp", _dp), ("x", _dp), ("obj", _dp), ("status", _ip),
                ("iters", _ip), ("sel", _ip), ("obstacles_version", ctypes.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Batch12), *args, **kw)


class Sim12(ctypes.Structure):
    """Mirror of srb12_sim (the closed-loop rollout of the SRB-12 mode; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("state", _dp), ("goal", _dp), ("phase", _ip),
                ("vref", ctypes.c_double), ("hcom", ctypes.c_double), ("yaw_step", ctypes.c_double),
                ("hold_radius", ctypes.c_double), ("gait", ctypes.c_int), ("c_first", ctypes.c_int),
                ("x", _dp), ("status", _ip), ("iters", _ip),
                ("x0", _dp), ("xref", _dp), ("foot", _dp), ("contact", _ip), ("last_state", _dp), ("com", _dp),
                ("traj", _dp), ("status_log", _ip), ("iters_log", _ip), ("x_log", _dp),
                ("obstacles", _dp), ("nbr_state", _dp),
                ("n_obs", ctypes.c_int), ("n_all", ctypes.c_int), ("agent_offset", ctypes.c_int),
                ("d_obs", _dp), ("d_agent", _dp), ("min_d_obs", _dp), ("min_d_agent", _dp), ("fail_cycle", _ip),
                ("distance_to_fail", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Sim12), *args, **kw)


class Plans12(ctypes.Structure):
    """Mirror of srb12_plans (the neighbour plans of the SRB-12 mode; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("nbr_plan", _dp), ("plan", _dp), ("plan_selection", ctypes.c_int),
                ("plan_table", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Plans12), *args, **kw)


class PlantStruct12(ctypes.Structure):
    """Mirror of srb12_plant (the disturbed plant of the SRB-12 rollout; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("seed", ctypes.c_ulonglong), ("kick_v", _dp), ("kick_p", _dp),
                ("kick_w", _dp), ("plant_mass", _dp), ("plant_inertia", _dp), ("at_state", ctypes.c_int),
                ("n_push", ctypes.c_int), ("push_cycle", _ip), ("push_agent", _ip), ("push_dv", _dp), ("dist_log", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(PlantStruct12), *args, **kw)


class Plant12:
    """The disturbed plant of a Rollout12 (srb12_plant; Rollout12(..., plant=Plant12(...))): from the second cycle on
    the state that starts a cycle is z + d instead of the model's prediction.

    seed      the key of the kicks' draws (0 .. 2^64 - 1): a rollout is reproducible per seed, and a LIP Rollout with
              the same plant_seed, kick_v and kick_p draws the same planar kicks
    kick_v, kick_p, kick_w   [A] float64 or None: the bounds (m/s, m, rad/s; finite, >= 0) of a uniform kick per cycle on
              (v_x, v_y), (p_x, p_y) and the three components of omega
    mass      [A] or None: the mass (kg, finite, > 0) of each agent's body (None: the model's)
    inertia   [A] or None: a factor (finite, > 0) on the model's body inertia (None: 1).  With either, z is the four-step
              roll of that body under the forces, footholds and contact flags the model applied
    at_state  True: every step of the roll evaluates the model's equations at the plant's own yaw and position
              instead of the model's linearisation point (the start state, then the reference)
    pushes    (cycle [P] int32, agent [P] int32, dv [P][6] float64) or None, P <= 4096: push p adds dv[p][0:3] to v and
              dv[p][3:6] to omega of agent[p] at the start of cycle[p] (cycles count from 0 at reset(); cycle 0 never
              fires: the start state is the caller's)
    All tensors are contiguous and on the solver's device (the device is checked by Rollout12, which also checks
    that every table has A rows).  Nothing set -- Plant12() -- is the nominal plant: the launches and bits of a
    Rollout12 without one."""

    def __init__(self, seed: int = 0, kick_v=None, kick_p=None, kick_w=None, mass=None, inertia=None,
                 at_state: bool = False, pushes=None):
        import torch
        seed = int(seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError("Plant12: seed must be 0 .. 2^64 - 1 (the 64-bit Philox key)")
        for name, tab in (("kick_v", kick_v), ("kick_p", kick_p), ("kick_w", kick_w), ("mass", mass),
                          ("inertia", inertia)):
            if tab is None:
                continue
            if not isinstance(tab, torch.Tensor) or tab.dtype != torch.float64 or tab.dim() != 1 or not tab.is_contiguous():
                raise ValueError(f"Plant12: {name} must be a contiguous float64 tensor [A], got "
                                 f"{getattr(tab, 'dtype', type(tab).__name__)} {tuple(getattr(tab, 'shape', ()))}")
            if bool(tab.isnan().any()):
                raise ValueError(f"Plant12: {name} holds a NaN")
            if not bool(tab.isfinite().all()):
                raise ValueError(f"Plant12: {name} must be finite")
            if name in ("mass", "inertia"):
                if bool((tab <= 0).any()):
                    raise ValueError(f"Plant12: {name} must be > 0 ({'kg' if name == 'mass' else 'a factor on I_b'})")
            elif bool((tab < 0).any()):
                raise ValueError(f"Plant12: {name} must be >= 0 (the bound of a uniform kick)")
        if pushes is not None:
            if not isinstance(pushes, (tuple, list)) or len(pushes) != 3:
                raise ValueError("Plant12: pushes must be a triple (cycle int32 [P], agent int32 [P], dv float64 [P][6])")
            cyc, agent, dv = pushes
            P = int(cyc.shape[0]) if hasattr(cyc, "shape") and len(cyc.shape) == 1 else -1
            if P < 0 or P > 4096:
                raise ValueError("Plant12: pushes: cycle must be an int32 tensor [P], P <= 4096")
            for name, t, shape, dt in (("cycle", cyc, (P,), torch.int32), ("agent", agent, (P,), torch.int32),
                                       ("dv", dv, (P, 6), torch.float64)):
                if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"Plant12: pushes: {name} must be a contiguous {dt} tensor of shape {shape}, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
            if P and bool(dv.isnan().any()):
                raise ValueError("Plant12: pushes: dv holds a NaN")
            pushes = (cyc, agent, dv) if P else None
        self.seed, self.kick_v, self.kick_p, self.kick_w, self.mass, self.inertia = seed, kick_v, kick_p, kick_w, mass, inertia
        self.at_state, self.pushes = bool(at_state), pushes

    @property
    def rolls(self) -> bool:
        """z is the four-step roll of the plant's own body (else the model's prediction)."""
        return self.mass is not None or self.inertia is not None or self.at_state

    @property
    def on(self) -> bool:
        """The plant is disturbed at all (else every call is the nominal one)."""
        return (self.kick_v is not None or self.kick_p is not None or self.kick_w is not None or self.rolls
                or self.pushes is not None)

    def check(self, A: int, device):
        """The checks that need the rollout: every table of A rows and, as the push tensors, on `device`; the pushed
        agents are rows 0 .. A - 1.  By name."""
        for name in ("kick_v", "kick_p", "kick_w", "mass", "inertia"):
            tab = getattr(self, name)
            if tab is None:
                continue
            if tab.shape[0] != A:
                raise ValueError(f"Plant12: {name} must have one row per agent ({A}), got {tab.shape[0]}")
            if tab.device != device:
                raise ValueError(f"Plant12: {name} must be on {device}, got {tab.device}")
        if self.pushes is not None:
            for name, t in zip(("cycle", "agent", "dv"), self.pushes):
                if t.device != device:
                    raise ValueError(f"Plant12: pushes: {name} must be on {device}, got {t.device}")
            agent = self.pushes[1]
            if bool((agent < 0).any()) or bool((agent >= A).any()):
                raise ValueError(f"Plant12: pushes: agent must be a row 0 .. {A - 1}")


GAITS = {"trot": 0, "stand": 1}       # srb12_sim.gait
SHIFT_GRIDS = 4                       # grids a cycle (one gait domain): the shift of the plans between cycles

_bound = False


def _lib():
    global _bound
    L = lib()
    if not _bound:
        L.srb12_params_default.argtypes = [ctypes.POINTER(Params12), ctypes.c_int]
        L.srb12_lds_bytes.argtypes = [ctypes.POINTER(Params12)]
        L.srb12_ctx_last_kernel.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)]
        L.srb12_kernel_table.argtypes = [ctypes.c_int, _ip, ctypes.POINTER(ctypes.c_char_p)]
        L.srb12_pick_kernel.argtypes = [ctypes.c_int, ctypes.c_int, _ip]
        L.srb12_check_params.argtypes = [ctypes.POINTER(Params12)]
        L.srb12_ctx_create.argtypes = [ctypes.POINTER(Params12), ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_void_p)]
        L.srb12_ctx_destroy.argtypes = [ctypes.c_void_p]
        L.srb12_solve_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12)]
        L.srb12_solve_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12), ctypes.c_void_p]
        L.srb12_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.srb12_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.srb12_ctx_set_scenes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.srb12_ctx_scenes.argtypes = [ctypes.c_void_p, _ip, _ip]
        for f in ("srb12_sim_advance_device", "srb12_sim_metrics_device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Sim12), ctypes.c_int, ctypes.c_void_p]
        L.srb12_rollout_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12), ctypes.POINTER(Sim12),
                                           ctypes.c_int, ctypes.c_void_p]
        L.srb12_solve_batch_plans.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                              ctypes.POINTER(Plans12)]
        L.srb12_solve_batch_plans_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                                     ctypes.POINTER(Plans12), ctypes.c_void_p]
        L.srb12_shift_plans_device.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, ctypes.c_int, _dp, ctypes.c_void_p]
        L.srb12_rollout_plans_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                                 ctypes.POINTER(Sim12), ctypes.POINTER(Plans12), ctypes.c_int,
                                                 ctypes.c_void_p]
        L.srb12_solve_batch_moving.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                               ctypes.POINTER(Plans12), ctypes.POINTER(Moving)]
        L.srb12_solve_batch_moving_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                                      ctypes.POINTER(Plans12), ctypes.POINTER(Moving), ctypes.c_void_p]
        L.srb12_obstacles_advance_device.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, _dp, ctypes.c_void_p]
        L.srb12_rollout_moving_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch12),
                                                  ctypes.POINTER(Sim12), ctypes.POINTER(Plans12), ctypes.POINTER(Moving),
                                                  ctypes.c_int, ctypes.c_void_p]
        B, S, PL, MV, SZ = (ctypes.POINTER(t) for t in (Batch12, Sim12, Plans12, Moving, Sizes))
        L.srb12_solve_batch_sized.argtypes = [ctypes.c_void_p, ctypes.c_int, B, PL, MV, SZ]
        L.srb12_solve_batch_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, PL, MV, SZ, ctypes.c_void_p]
        L.srb12_sim_metrics_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, S, SZ, ctypes.c_int, ctypes.c_void_p]
        L.srb12_rollout_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, S, PL, MV, SZ, ctypes.c_int,
                                                 ctypes.c_void_p]
        AG = ctypes.POINTER(AgentSizes)
        L.srb12_solve_batch_agents.argtypes = [ctypes.c_void_p, ctypes.c_int, B, PL, MV, SZ, AG]
        L.srb12_solve_batch_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, PL, MV, SZ, AG, ctypes.c_void_p]
        L.srb12_sim_metrics_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, S, SZ, AG, ctypes.c_int,
                                                      ctypes.c_void_p]
        L.srb12_rollout_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, S, PL, MV, SZ, AG, ctypes.c_int,
                                                  ctypes.c_void_p]
        PT = ctypes.POINTER(PlantStruct12)
        L.srb12_sim_advance_plant_device.argtypes = [ctypes.c_void_p, ctypes.c_int, S, PT, ctypes.c_int, ctypes.c_void_p]
        L.srb12_rollout_plant_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, S, PL, MV, SZ, AG, PT, ctypes.c_int,
                                                 ctypes.c_void_p]
        LN = ctypes.POINTER(Link)
        L.srb12_link_update_device.argtypes = [ctypes.c_void_p, ctypes.c_int, LN, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p]
        L.srb12_solve_batch_link_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, PL, MV, SZ, AG, _dp, ctypes.c_void_p]
        L.srb12_rollout_link_device.argtypes = [ctypes.c_void_p, ctypes.c_int, B, S, PL, MV, SZ, AG, PT, LN, ctypes.c_int,
                                                ctypes.c_void_p]
        _bound = True
    return L


def default_params(N: int = 10, **overrides) -> Params12:
    p = Params12()
    _lib().srb12_params_default(ctypes.byref(p), N)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def lds_bytes(p: Params12) -> int:
    return _lib().srb12_lds_bytes(ctypes.byref(p))


def check_params(p: Params12) -> bool:
    """True where srb12_ctx_create would accept p (srb12_check_params; no device needed)."""
    return _lib().srb12_check_params(ctypes.byref(p)) == 0


def kernel_table():
    """The shipped SRB-12 solve-kernel instances (srb12_kernel_table; no device needed): a list of
    ((TL, TO, NC, K1), solve kernel name)."""
    out = []
    while True:
        d = (ctypes.c_int * 4)(); name = ctypes.c_char_p()
        if _lib().srb12_kernel_table(len(out), d, ctypes.byref(name)) != 0:
            return out
        out.append((tuple(d), name.value.decode()))


def pick_kernel(N: int, K: int):
    """(TL, TO, NC, K1) of the instance that horizon N with K rows per grid picks (srb12_pick_kernel; no device
    needed); raises where no instance fits."""
    d = (ctypes.c_int * 4)()
    _check(_lib().srb12_pick_kernel(int(N), int(K), d))
    return tuple(d)


def n_selected(p: Params12, n_obs: int, n_all: int, scenes=(0, 0)):
    """(Ko, Kn) rows selected per agent for tables of these sizes (clamped as the C ABI does; with a scene
    partition (scene_agents, scene_obs) to the agent's scene)."""
    return _clamp_selected(p.K_obs, p.K_nbr, n_obs, n_all, scenes) if p.use_nlp else (0, 0)


class Solver12(_SolverBase):
    """One HIP context solving SRB-12 batches of up to `max_agents` agents."""
    _abi = "srb12"
    _lib = staticmethod(_lib)

    def solve(self, x0, xref, foot, contact, obstacles=None, nbr_state=None, agent_offset: int = 0, nbr_plan=None,
              plan_selection: bool = False, obs_vel=None, obs_horizon: bool = False, obs_eps=None,
              obs_clearance: bool = False, agent_rad=None, agent_pad=None, nbr_clearance: bool = False):
        """Host numpy: x0 [A,12], xref [A,N,12], foot [A,N,4,3], contact [A,N,4] int.  Returns
        dict x_qp, x [A, 24N+1], obj, status [A,2], iters [A,2], sel [A, Ko+Kn], plan [A,N,2] (the (x, y) of
        X at every grid).  nbr_plan ([n_all][N][2], float64, C-contiguous) makes the neighbour rows follow the
        neighbours' plans instead of the constant-velocity guess; plan_selection selects the neighbours by
        closest predicted approach over the horizon (needs nbr_plan).  obs_vel ([n_obs][2], float64, C-contiguous): the
        obstacles move at these velocities over the horizon (srb12_solve_batch_moving); obs_horizon=True additionally
        selects the static columns by closest predicted approach (needs obs_vel).  obs_eps ([n_obs], float64,
        C-contiguous): the CBF level of each obstacle row in squared metres, the unit of eps_obs
        (srb12_solve_batch_sized); obs_clearance=True additionally selects the static columns by clearance to the level
        set (needs obs_eps).  agent_rad, agent_pad ([n_all], float64, C-contiguous, finite; agent_rad >= 0): a safety
        radius and a pad per row of nbr_state (srb12_solve_batch_agents): neighbour column j at the level
        (agent_rad[g] + agent_rad[sel[j]])^2, every static column of agent g at (sqrt(level) + agent_pad[g])^2;
        nbr_clearance=True additionally selects the neighbour columns by clearance dist - agent_rad (needs agent_rad)."""
        p = self.params
        x0 = np.ascontiguousarray(x0, np.float64); A = x0.shape[0]
        xref = np.ascontiguousarray(xref, np.float64); foot = np.ascontiguousarray(foot, np.float64)
        contact = np.ascontiguousarray(contact, np.int32)
        ob = np.ascontiguousarray(obstacles if obstacles is not None else np.zeros((0, 2)), np.float64)
        nb = np.ascontiguousarray(nbr_state, np.float64) if nbr_state is not None else None
        Ko, Kn = n_selected(p, ob.shape[0], nb.shape[0] if nb is not None else 0, self._scenes)
        out = dict(x_qp=np.zeros((A, p.nv)), x=np.zeros((A, p.nv)), obj=np.zeros(A),
                   status=np.zeros((A, 2), np.int32), iters=np.zeros((A, 2), np.int32),
                   sel=np.full((A, Ko + Kn), -2, np.int32))
        b = Batch12(_p(x0), _p(xref), _p(foot), _p(contact), _p(ob) if ob.shape[0] else None,
                    _p(nb) if nb is not None else None, ob.shape[0], nb.shape[0] if nb is not None else 0,
                    int(agent_offset), _p(out["x_qp"]), _p(out["x"]), _p(out["obj"]), _p(out["status"]),
                    _p(out["iters"]), _p(out["sel"]) if out["sel"].size else None, 0)
        if nbr_plan is not None:
            # (without nbr_state the row count is the table's own: the library refuses that call by name)
            _check_plan_array(nbr_plan, (nb.shape[0] if nb is not None else len(nbr_plan), p.N, 2), "nbr_plan", np.float64)
        out["plan"] = np.zeros((A, p.N, 2))
        pl = Plans12(_p(nbr_plan) if nbr_plan is not None else None, _p(out["plan"]), 1 if plan_selection else 0, None)
        moving = obs_vel is not None or obs_horizon
        mv = _moving_args(obs_vel, obs_horizon, ob.shape[0], np.float64, _p, p.use_nlp) if moving else None
        if agent_rad is not None or agent_pad is not None or nbr_clearance:
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, ob.shape[0], np.float64, _p, p.use_nlp) if sized else None
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, nb.shape[0] if nb is not None else 0, np.float64,
                             _p, p.use_nlp)
            _check(_lib().srb12_solve_batch_agents(self._h, A, ctypes.byref(b), ctypes.byref(pl),
                                                   ctypes.byref(mv) if moving else None,
                                                   ctypes.byref(sz) if sized else None, ctypes.byref(ag)))
            return out
        if obs_eps is not None or obs_clearance:
            sz = _sizes_args(obs_eps, None, obs_clearance, ob.shape[0], np.float64, _p, p.use_nlp)
            _check(_lib().srb12_solve_batch_sized(self._h, A, ctypes.byref(b), ctypes.byref(pl),
                                                  ctypes.byref(mv) if moving else None, ctypes.byref(sz)))
            return out
        if moving:
            _check(_lib().srb12_solve_batch_moving(self._h, A, ctypes.byref(b), ctypes.byref(pl), ctypes.byref(mv)))
            return out
        _check(_lib().srb12_solve_batch_plans(self._h, A, ctypes.byref(b), ctypes.byref(pl)))
        return out

    def solve_device(self, x0, xref, foot, contact, obstacles, nbr_state, out, agent_offset: int = 0, stream=None,
                     obstacles_version: int = 0, nbr_plan=None, plan_selection: bool = False, plan=None, obs_vel=None,
                     obs_horizon: bool = False, obs_eps=None, obs_clearance: bool = False, agent_rad=None, agent_pad=None,
                     nbr_clearance: bool = False, own_plan=None):
        """torch tensors on this device (float64 / int32), contiguous; out holds x_qp (or None), x, obj,
        status, iters and optionally sel [A, Ko+Kn] and plan [A, N, 2] (written when the key is present; the
        `plan` argument overrides it).  nbr_plan ([n_all][N][2] float64, contiguous): the neighbours' plans for the
        inter-agent rows (None: constant velocity), must not overlap plan; plan_selection: the neighbours by
        closest predicted approach (needs nbr_plan).  obs_vel ([n_obs][2] float64, contiguous): the obstacles'
        velocities (srb12_solve_batch_moving_device; needs obstacles_version 0); obs_horizon=True selects the static
        columns by closest predicted approach (needs obs_vel).  obs_eps ([n_obs] float64, contiguous): the CBF level of
        each obstacle row (srb12_solve_batch_sized_device; goes together with obstacles_version); obs_clearance=True
        selects the static columns by clearance to the level set (needs obs_eps).  agent_rad, agent_pad ([n_all]
        float64, contiguous, finite; agent_rad >= 0): a safety radius and a pad per row of nbr_state
        (srb12_solve_batch_agents_device; the values of a tensor are looked at once, on its first use with this solver);
        nbr_clearance=True selects the neighbour columns by clearance dist - agent_rad (needs agent_rad).  own_plan
        ([A][N][2] float64, contiguous; needs plan_selection, must not overlap plan, not with nbr_clearance): the agents'
        own plans for the horizon-aware selection, which otherwise reads row agent_offset + a of nbr_plan -- for a table
        that is what the agent perceives of its neighbours (srb12_solve_batch_link_device).  Asynchronous on `stream`
        (default: torch's current)."""
        A = x0.shape[0]
        import torch
        Ko, Kn = n_selected(self.params, 0 if obstacles is None else obstacles.shape[0],
                            0 if nbr_state is None else nbr_state.shape[0], self._scenes)
        sel = out.get("sel")
        # the kernel writes rows of stride Ko + Kn (clamped to the tables, 0 without the NLP stage):
        # anything else would be overrun or read misaligned (BatchSolver.solve_device, same check)
        if sel is not None and (sel.dtype != torch.int32 or tuple(sel.shape) != (A, Ko + Kn) or not sel.is_contiguous()):
            raise ValueError(f"out['sel'] must be a contiguous int32 tensor of shape ({A}, {Ko + Kn}) "
                             f"(n_selected(params, n_obs, n_all)), got {tuple(sel.shape)} {sel.dtype}")
        b = Batch12(_dptr(x0), _dptr(xref), _dptr(foot), _iptr(contact), _dptr(obstacles), _dptr(nbr_state),
                    0 if obstacles is None else obstacles.shape[0], 0 if nbr_state is None else nbr_state.shape[0],
                    int(agent_offset), _dptr(out.get("x_qp")), _dptr(out["x"]), _dptr(out["obj"]), _iptr(out["status"]),
                    _iptr(out["iters"]), _iptr(sel), int(obstacles_version))
        if plan is None:
            plan = out.get("plan")
        N = self.params.N
        if nbr_plan is not None:
            _check_plan_array(nbr_plan, (nbr_plan.shape[0] if nbr_state is None else nbr_state.shape[0], N, 2),
                              "nbr_plan", torch.float64)
        if plan is not None:
            _check_plan_array(plan, (A, N, 2), "plan", torch.float64)
        no_plans = nbr_plan is None and plan is None and not plan_selection
        n_obs = 0 if obstacles is None else obstacles.shape[0]
        moving = obs_vel is not None or obs_horizon
        mv = _moving_args(obs_vel, obs_horizon, n_obs, torch.float64, _dptr, self.params.use_nlp) if moving else None
        if own_plan is not None:                 # the entry point of its own; without, every launch as before
            _check_plan_array(own_plan, (A, N, 2), "own_plan", torch.float64)
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch.float64, _dptr, self.params.use_nlp,
                             device=x0.device) if sized else None
            agents = agent_rad is not None or agent_pad is not None or nbr_clearance
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, 0 if nbr_state is None else nbr_state.shape[0],
                             torch.float64, _dptr, self.params.use_nlp, device=x0.device,
                             checked=self._agent_checked()) if agents else None
            pl = None if no_plans else ctypes.byref(Plans12(_dptr(nbr_plan), _dptr(plan), 1 if plan_selection else 0, None))
            _check(_lib().srb12_solve_batch_link_device(self._h, A, ctypes.byref(b), pl,
                                                        ctypes.byref(mv) if moving else None,
                                                        ctypes.byref(sz) if sized else None,
                                                        ctypes.byref(ag) if agents else None, _dptr(own_plan),
                                                        self._stream(stream)))
            return
        if agent_rad is not None or agent_pad is not None or nbr_clearance:
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch.float64, _dptr, self.params.use_nlp,
                             device=x0.device) if sized else None
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, 0 if nbr_state is None else nbr_state.shape[0],
                             torch.float64, _dptr, self.params.use_nlp, device=x0.device, checked=self._agent_checked())
            pl = None if no_plans else ctypes.byref(Plans12(_dptr(nbr_plan), _dptr(plan), 1 if plan_selection else 0, None))
            _check(_lib().srb12_solve_batch_agents_device(self._h, A, ctypes.byref(b), pl,
                                                          ctypes.byref(mv) if moving else None,
                                                          ctypes.byref(sz) if sized else None, ctypes.byref(ag),
                                                          self._stream(stream)))
            return
        if obs_eps is not None or obs_clearance:
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch.float64, _dptr, self.params.use_nlp, device=x0.device)
            pl = None if no_plans else ctypes.byref(Plans12(_dptr(nbr_plan), _dptr(plan), 1 if plan_selection else 0, None))
            _check(_lib().srb12_solve_batch_sized_device(self._h, A, ctypes.byref(b), pl,
                                                         ctypes.byref(mv) if moving else None, ctypes.byref(sz),
                                                         self._stream(stream)))
            return
        if moving:
            pl = None if no_plans else ctypes.byref(Plans12(_dptr(nbr_plan), _dptr(plan), 1 if plan_selection else 0, None))
            _check(_lib().srb12_solve_batch_moving_device(self._h, A, ctypes.byref(b), pl, ctypes.byref(mv),
                                                          self._stream(stream)))
            return
        if no_plans:
            _check(_lib().srb12_solve_batch_device(self._h, A, ctypes.byref(b), self._stream(stream)))
            return
        pl = Plans12(_dptr(nbr_plan), _dptr(plan), 1 if plan_selection else 0, None)
        _check(_lib().srb12_solve_batch_plans_device(self._h, A, ctypes.byref(b), ctypes.byref(pl), self._stream(stream)))

    def shift_plans_device(self, plan, table, grids: int = SHIFT_GRIDS, stream=None):
        """dist.shift_plans on the device (srb12_shift_plans_device): table[a][k] = plan[a][k + grids], past the
        horizon along the last finite difference.  plan, table [A][N][2] float64 on this device, two buffers."""
        import torch
        A = plan.shape[0] if hasattr(plan, "shape") and len(plan.shape) == 3 else -1
        _check_plan_array(plan, (A, self.params.N, 2), "plan", torch.float64)
        _check_plan_array(table, (A, self.params.N, 2), "table", torch.float64)
        _check(_lib().srb12_shift_plans_device(self._h, A, _dptr(plan), int(grids), _dptr(table), self._stream(stream)))

    def advance_obstacles_device(self, obstacles, obs_vel, stream=None):
        """One control cycle (4 grids) of a moving obstacle table, in place (srb12_obstacles_advance_device):
        obstacles[i] += obs_vel[i] * (Ts * 4).  Both [n_obs][2] float64 tensors on this solver's device."""
        import torch
        n = obstacles.shape[0] if hasattr(obstacles, "shape") and len(obstacles.shape) else -1
        _check_vel_array(obstacles, n, torch.float64, "obstacles")
        _check_vel_array(obs_vel, n, torch.float64)
        _check(_lib().srb12_obstacles_advance_device(self._h, n, _dptr(obstacles), _dptr(obs_vel), self._stream(stream)))

    def solve_coupled_device(self, x0, xref, foot, contact, obstacles, nbr_state, out, outer: int = 2, exchange=None,
                             nbr_plan=None, agent_offset: int = 0, stream=None, obstacles_version: int = 0,
                             plan_selection: bool = False, obs_vel=None, obs_horizon: bool = False, obs_eps=None,
                             obs_clearance: bool = False, agent_rad=None, agent_pad=None, nbr_clearance: bool = False):
        """Jacobi iteration over the agents' plans (BatchSolver.solve_coupled_device for the 12-state body):
        `outer` solves of the same cycle, each against the plans the agents wrote in the round before.  Round 0
        solves against nbr_plan (None: the constant-velocity rows); every later round r reads table =
        exchange(plan of round r - 1), a dist.PlanExchange, or on one GPU (exchange None: the batch is the whole
        team, agent_offset 0) that plan tensor itself.  The plans ping-pong between out["plan"] ([A][N][2],
        required) and a second buffer of this solver; the last round's results are in `out`.  Returns
        plan_change, a device tensor [outer - 1]: max |plan_r - plan_{r-1}| per round (torch reductions; nothing
        synchronises with the host inside the loop).  plan_selection applies to every round that has a table; obs_vel,
        obs_horizon, obs_eps, obs_clearance, agent_rad, agent_pad and nbr_clearance as solve_device (every round solves
        against the same obstacle and agent tables)."""
        return self._solve_coupled((x0, xref, foot, contact, obstacles, nbr_state, out), outer, exchange, nbr_plan,
                                   agent_offset, stream,
                                   lambda table: {"plan_selection": plan_selection and table is not None},
                                   obstacles_version=obstacles_version, obs_vel=obs_vel, obs_horizon=obs_horizon,
                                   obs_eps=obs_eps, obs_clearance=obs_clearance, agent_rad=agent_rad, agent_pad=agent_pad,
                                   nbr_clearance=nbr_clearance)

    def last_kernel(self) -> str:
        """Name of the solve kernel the last launch ran (srb12_ctx_last_kernel)."""
        a = ctypes.c_char_p()
        _check(_lib().srb12_ctx_last_kernel(self._h, ctypes.byref(a)))
        return a.value.decode()

    def last_kernel_ms(self):
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(_lib().srb12_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_timing(self, on: bool):
        """HIP events around the kernels (srb12_ctx_set_timing; default on): last_kernel_ms needs them."""
        _check(_lib().srb12_ctx_set_timing(self._h, 1 if on else 0))


def split(p: Params12, x):
    """x [..., 24N+1] -> X [..., N, 12], U [..., N, 4, 3], s [...]"""
    N = p.N
    return (x[..., :12 * N].reshape(x.shape[:-1] + (N, 12)), x[..., 12 * N:24 * N].reshape(x.shape[:-1] + (N, 4, 3)),
            x[..., 24 * N])


class Rollout12(_RolloutBase):
    """The closed loop of `solver` (a Solver12 with N >= 4) for the agents whose goals are `goal` [A][2]
    (srb12_sim_advance_device / srb12_sim_metrics_device / srb12_rollout_device): srbnmpc.Rollout for the 12-state
    body, with the nominal plant (or, with plant=, a disturbed one), the goal-directed reference of workload.make_batch12 re-centred every cycle and
    the team's safety log.

        r = Rollout12(solver, goal, obstacles=obstacles)
        r.reset(state)              # [A][12] p, roll/pitch/yaw, v, omega
        r.run(50)                   # the C driver: no host round trip inside
        out = r.results()           # traj, status, iters, min_d_agent, min_d_obs, fail_cycle, ...

    vref        reference speed of the goal-directed line (workload.VREF)
    phase       [A] int32 or None: added to the cycle index for the trot parity
    gait        "trot" (one diagonal per gait domain) or "stand" (all four legs)
    log_x       True: keep every cycle's decision vectors (results()["x"], [T][A][24N+1])
    obstacles   [n_obs][2] or None: the static obstacles, for the solve and for d_obs / fail_cycle; with the
                solver's scene partition on (Solver12.set_scenes, inputs from workload.make_scenes12) the
                scene-major table [n_scenes * n_obs][2]
    hcom        reference CoM height
    yaw_step, hold_radius   the yaw reference turns towards the goal's bearing by at most yaw_step a cycle and
                keeps the yaw within hold_radius of the goal
    plans       True: from the second cycle on, the inter-agent rows follow the neighbours' previous plans shifted
                by one gait domain (srb12_plans.nbr_plan) instead of the constant-velocity guess; step() shifts
                with srb12_shift_plans_device, run() is srb12_rollout_plans_device, the same bits
    plan_selection  with plans: the neighbours by closest predicted approach, in every cycle that has a table
    obs_vel     [n_obs][2] or None: the obstacles' velocities (m/s).  The rollout then clones `obstacles` (it moves the
                table: from the second cycle on by obs_vel * (Ts * 4) before the metrics), reset() restores the clone,
                results()["obstacles"] is the current table; run() is srb12_rollout_moving_device
    obs_horizon True: the static columns by closest predicted approach over the horizon (needs obs_vel)
    obs_eps     [n_obs] or None: the CBF level of each obstacle row, squared metres (None: eps_obs for every row)
    obs_radius  [n_obs] or None: the body radius (m) of each obstacle row: d_obs is then min_i (dist_i - obs_radius[i])
                on the CoM rows and fail_cycle the first cycle with d_obs < 0 (None: centre distances and the 0.5 m test)
    obs_clearance  True: the static columns by clearance to the level set (needs obs_eps).  With any of the three run()
                is srb12_rollout_sized_device; the tables do not change over a rollout
    agent_rad   [A] or None: the safety radius (m) of each agent: neighbour column j of agent g at the level
                (agent_rad[g] + agent_rad[sel[j]])^2 (None: eps_nbr for every pair)
    agent_pad   [A] or None: metres added to the safety radius of every static column of each agent
    agent_body  [A] or None: the body radius (m) of each agent: d_agent is then
                min_i (dist_i - (agent_body[g] + agent_body[i])) on the CoM rows, results() gains collide_cycle (the first
                cycle with d_agent < 0, else -1) and scene_results() n_collided (None: centre distances)
    nbr_clearance  True: the neighbour columns by clearance dist - agent_rad (needs agent_rad).  With any of the three
                tables run() is srb12_rollout_agents_device; the tables are finite, agent_rad and agent_body not
                negative, and do not change over a rollout
    plant       a Plant12 or None: the disturbed plant (srb12_plant) -- kicks on v, p and omega, pushes, a body of
                another mass or inertia, or the model's equations evaluated at the plant's own state.  advance(), step()
                and run() then go through srb12_sim_advance_plant_device / srb12_rollout_plant_device (the same bits),
                and results() gains disturbance [T][A][12] (state order; row c - 1 is what the start of cycle c added).
                None, or a Plant12 with nothing set: the nominal plant, the launches and bits as ever.  The LIP
                rollout's keyword arguments plant_seed, kick_v, kick_p, plant_hcom and pushes are refused by name
    link        None or a srbnmpc.LinkModel: the degraded neighbour link (srb_link; rollout.Rollout's argument, the same
                tables, checks and draws).  With any table set the solve and its selection read seen_state [A][4] /
                seen_plan [A][N][2] (attributes, readable after a step) instead of the truth; the metrics and the logs
                keep the truth, results() gains link_age [T][A], and reset() restarts the link.  step() goes through
                srb12_link_update_device and srb12_solve_batch_link_device, run() through srb12_rollout_link_device (the
                same bits).  plan_selection goes together with it: the selection then takes each agent's own plan from
                the truth (plan_table), not from its row of the perceived table.  Not with nbr_clearance and
                plan_selection together (refused by name).  None, or a LinkModel with nothing set: the launches and bits
                as ever
    A whole team on one GPU (the SRB-12 mode has no sharded stepping).  All tensors are
    float64 / int32, contiguous, on the solver's device.  Cycles count from 0 at reset()."""
    _nx = 12
    _name = "Rollout12"

    def __init__(self, solver, goal, vref: float = 0.27, phase=None, gait: str = "trot", log_x: bool = False,
                 obstacles=None, hcom: float = workload.HCOM12, yaw_step: float = 0.1, hold_radius: float = 0.05,
                 plans: bool = False, plan_selection: bool = False, obs_vel=None, obs_horizon: bool = False,
                 obs_eps=None, obs_radius=None, obs_clearance: bool = False, agent_rad=None, agent_pad=None,
                 agent_body=None, nbr_clearance: bool = False, *, plant=None, plant_seed: int = 0, kick_v=None,
                 kick_p=None, plant_hcom=None, pushes=None, link=None):
        import torch
        for name, arg in (("plant_seed", plant_seed or None), ("kick_v", kick_v), ("kick_p", kick_p),
                          ("plant_hcom", plant_hcom), ("pushes", pushes)):
            if arg is not None:
                raise ValueError(f"Rollout12: {name} is not available: it is an argument of the LIP rollout's plant "
                                 "(rollout.Rollout); the SRB-12 mode takes plant=Plant12(...) (srb12.Plant12: seed, kick_v, "
                                 "kick_p, kick_w, mass, inertia, at_state, pushes)")
        if plant is not None and not isinstance(plant, Plant12):
            raise ValueError(f"Rollout12: plant must be a srb12.Plant12 or None, got {type(plant).__name__}")
        if gait not in GAITS:
            raise ValueError(f"gait must be one of {sorted(GAITS)}, got {gait!r}")
        super().__init__(solver, goal, vref, phase, plans, log_x, obstacles, obs_vel, obs_horizon, obs_eps, obs_radius,
                         obs_clearance)
        self._set_agent_sizes(agent_rad, agent_pad, agent_body, nbr_clearance, self.A)
        self._set_link(link, self.A)
        self.gait, self.hcom = gait, float(hcom)
        self.plan_selection = bool(plan_selection)
        if self.plan_selection and not self.plans:
            raise ValueError("plan_selection needs plans=True (the horizon-aware selection reads the plan table)")
        if self.link is not None and self.plan_selection and self.nbr_clearance:
            raise ValueError("link with plan_selection and nbr_clearance: the clearance selection reads the agent's own plan "
                             "from its row of the perceived table (not built)")
        self.yaw_step, self.hold_radius = float(yaw_step), float(hold_radius)
        A, N = self.A, solver.params.N
        f8 = dict(dtype=torch.float64, device=self.device)
        self.com = torch.zeros((A, 4), **f8)
        self.xref = torch.zeros((A, N, 12), **f8)
        self.foot = torch.zeros((A, N, 4, 3), **f8)
        self.contact = torch.zeros((A, N, 4), dtype=torch.int32, device=self.device)
        if plant is not None:
            plant.check(A, self.device)
        self.plant = plant if plant is not None and plant.on else None
        self.dist_log = None
        self._advanced = -1             # the cycle whose advance has run (the plant's advance is not idempotent)

    # ------------------------------------------------------------------ the disturbed plant (srb12_plant)
    def _plant(self) -> PlantStruct12:
        pt = self.plant
        cyc, agent, dv = pt.pushes if pt.pushes is not None else (None, None, None)
        return PlantStruct12(pt.seed, _dptr(pt.kick_v), _dptr(pt.kick_p), _dptr(pt.kick_w), _dptr(pt.mass),
                             _dptr(pt.inertia), int(pt.at_state), 0 if cyc is None else cyc.shape[0], _iptr(cyc),
                             _iptr(agent), _dptr(dv), _dptr(self.dist_log))

    def _reserve(self, cycles: int):
        super()._reserve(cycles)
        if self.plant is not None and (self.dist_log is None or self.dist_log.shape[0] < self.cap):
            import torch
            new = torch.zeros((self.cap, self.A, 12), dtype=torch.float64, device=self.device)
            if self.dist_log is not None:
                new[:self.dist_log.shape[0]] = self.dist_log
            self.dist_log = new

    def reset(self, state):
        super().reset(state)
        self._advanced = -1               # (dist_log needs no clearing: results() returns the rows rewritten since)

    def advance(self, stream=None):
        """As _RolloutBase.advance; with a disturbed plant through srb12_sim_advance_plant_device, and once per cycle:
        the plant rolls on from the state and the inputs of the previous cycle, which the advance overwrites, so a
        second call for the same cycle is skipped (everything it would write is already there)."""
        if self.plant is None:
            return super().advance(stream)
        if not self._ready:
            raise RuntimeError("Rollout12.advance before reset(state)")
        if self._advanced == self.c:
            return
        s = self.solver
        self._reserve(self.c + 1)
        _check(_lib().srb12_sim_advance_plant_device(s._h, self.A, ctypes.byref(self._sim()), ctypes.byref(self._plant()),
                                                     self.c, s._stream(stream)))
        self._advanced = self.c

    def results(self, stream=None):
        """As _RolloutBase.results; with a disturbed plant also disturbance [T][A][12]: row c - 1 is the d (state order:
        p, roll/pitch/yaw, v, omega) that the start of cycle c added to the plant's base state."""
        out = super().results(stream)
        if self.plant is not None:
            out["disturbance"] = self.dist_log[:self.c]
        return out

    def _sim(self) -> Sim12:
        m, o = self.metrics, self.out
        return Sim12(_dptr(self.state), _dptr(self.goal), _iptr(self.phase), self.vref, self.hcom, self.yaw_step,
                     self.hold_radius, GAITS[self.gait], 0, _dptr(o["x"]), _iptr(o["status"]), _iptr(o["iters"]),
                     _dptr(self.x0), _dptr(self.xref), _dptr(self.foot), _iptr(self.contact), _dptr(self.last_state),
                     _dptr(self.com), _dptr(self.traj), _iptr(self.status_log), _iptr(self.iters_log),
                     _dptr(self.x_log), _dptr(self.obstacles), _dptr(self.last_state),
                     0 if self.obstacles is None else self.obstacles.shape[0], self.A, 0,
                     _dptr(m["d_obs"]), _dptr(m["d_agent"]), _dptr(m["min_d_obs"]), _dptr(m["min_d_agent"]),
                     _iptr(m["fail_cycle"]), _dptr(m["distance_to_fail"]))

    def step(self, stream=None):
        """One cycle: advance, metrics, solve."""
        if not self._ready:
            raise RuntimeError("Rollout12.step before reset(state)")
        s = self.solver
        self._reserve(self.c + 1)
        self.advance(stream)
        if self.obs_vel is not None and self.c > 0:          # the obstacles' cycle, before the metrics read the table
            s.advance_obstacles_device(self.obstacles, self.obs_vel, stream)
        self._metrics(self._sim(), stream)
        table = self.plan_table if self.plans and self.c > 0 else None
        nbr, own = self.last_state, None
        if self.link is not None:                # the solve reads what is seen of the truth
            _check(_lib().srb12_link_update_device(s._h, self.A, ctypes.byref(self._link()), _dptr(self.last_state),
                                                   _dptr(table), self.c, 0, s._stream(stream)))
            nbr = self.seen_state
            if table is not None:                # ... and the selection its own plan from the truth
                own = self.plan_table if self.plan_selection else None
                table = self.seen_plan
        s.solve_device(self.x0, self.xref, self.foot, self.contact, self.obstacles, nbr, self.out,
                       stream=stream, nbr_plan=table, plan_selection=self.plan_selection and table is not None,
                       obs_vel=self.obs_vel, obs_horizon=self.obs_horizon, obs_eps=self.obs_eps,
                       obs_clearance=self.obs_clearance, agent_rad=self.agent_rad, agent_pad=self.agent_pad,
                       nbr_clearance=self.nbr_clearance, own_plan=own)
        if self.plans:
            s.shift_plans_device(self.out["plan"], self.plan_table, SHIFT_GRIDS, stream=stream)
        self.c += 1
        self.flushed = False

    def _drive(self, T: int, stream):
        s, o = self.solver, self.out
        b = Batch12(None, None, None, None, _dptr(self.obstacles), None,
                    0 if self.obstacles is None else self.obstacles.shape[0], self.A, 0,
                    None, _dptr(o["x"]), _dptr(o["obj"]), _iptr(o["status"]), _iptr(o["iters"]), None, 0)
        pl = None
        if self.plans:
            pl = ctypes.byref(Plans12(None, _dptr(o["plan"]), 1 if self.plan_selection else 0, _dptr(self.plan_table)))
        if self.link is not None:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            ag = ctypes.byref(self._agent_sizes()) if self.agents else None
            pt = ctypes.byref(self._plant()) if self.plant is not None else None
            _check(_lib().srb12_rollout_link_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl, mv, sz,
                                                    ag, pt, ctypes.byref(self._link()), T, s._stream(stream)))
            if self.plant is not None:
                self._advanced = T
        elif self.plant is not None:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            ag = ctypes.byref(self._agent_sizes()) if self.agents else None
            _check(_lib().srb12_rollout_plant_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl, mv, sz,
                                                     ag, ctypes.byref(self._plant()), T, s._stream(stream)))
            self._advanced = T               # the driver's final advance was cycle T's
        elif self.agents:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            sz = ctypes.byref(self._sizes()) if self.sized else None
            _check(_lib().srb12_rollout_agents_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl, mv, sz,
                                                      ctypes.byref(self._agent_sizes()), T, s._stream(stream)))
        elif self.sized:
            mv = ctypes.byref(self._moving()) if self.obs_vel is not None else None
            _check(_lib().srb12_rollout_sized_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl, mv,
                                                     ctypes.byref(self._sizes()), T, s._stream(stream)))
        elif self.obs_vel is not None:
            _check(_lib().srb12_rollout_moving_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl,
                                                      ctypes.byref(self._moving()), T, s._stream(stream)))
        elif self.plans:
            _check(_lib().srb12_rollout_plans_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), pl, T,
                                                     s._stream(stream)))
        else:
            _check(_lib().srb12_rollout_device(s._h, self.A, ctypes.byref(b), ctypes.byref(self._sim()), T,
                                               s._stream(stream)))
