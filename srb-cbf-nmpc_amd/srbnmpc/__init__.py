"""srbnmpc -- batched CBF-NMPC solver for MI355X, Python host side.

Thin ctypes layer over the C ABI in include/srbnmpc.h (libsrbnmpc.so, HIP kernels for
gfx950).  There is no CPU fallback: if the library is missing, or no GPU is visible,
constructing a solver raises.

    BatchSolver   -- whole agent batch per call (host numpy or device torch buffers)
    Rollout       -- closed-loop team rollout of a BatchSolver on the device (srbnmpc.rollout)
    MPCDist       -- per-agent object with the reference's MPC_dist call surface
                     (/root/reference/include/MPC_dist.hpp:137-190)
    workload      -- synthetic agent batches with the SURVEY.md §8d distributions
    LowLevelCtrl  -- batched low-level CLF-QP (LowLevelCtrl::calcTorque), srbnmpc.lowlevel
    ll_workload   -- synthetic A1-sized low-level controller inputs

What the LIP and the SRB-12 mode (srbnmpc.srb12) do alike is here once: _SolverBase under BatchSolver and
srb12.Solver12, the pointer casts _p / _dptr / _iptr, _clamp_selected and _moving_args.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# the product library; no environment variable can change it: a diagnostic A/B
# build is selected only by an explicit use_library() call (bench.py --lib, pytest --srbnmpc-lib)
LIB_PATH = os.path.join(_HERE, "libsrbnmpc.so")

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)

OPTIMAL, KKTFAIL, MAXIT, FATAL, ACCEPTABLE = 0, 1, 2, 3, 4
# status 4 means, by stage: NLP -- ACCEPTABLE (round-off floor, or a loosened exit whose polish was not
# accepted); QP stage followed by the NLP -- QP_WARM, converged at the warm-start tolerance (SRB_OPT_QP_WARM_TOL;
# x_qp is the NLP's warm start, not iSWIFT's 1e-6 point); the last stage of an SRB-12 solve -- its polish rejected
QP_WARM = 4
# srb_ctx_set_option codes (SRB_OPT_* of include/srbnmpc.h)
OPTIONS = {"polish": 1, "polish_rho": 2, "polish_waves": 3, "grid_min_rows": 4, "grid_min_rows_static": 5,
           "polish_fused": 6, "last_polish": 7, "timing": 8, "qp_warm_tol": 9, "selection": 10,
           "kkt_fp32_mu": 11, "kkt_fp32_refine": 12, "last_kkt_fp32": 13, "plan_selection": 14}
ABI_VERSION = 6                                               # SRB_ABI_VERSION of include/srbnmpc.h


class Params(ctypes.Structure):
    """Mirror of srb_params (include/srbnmpc.h)."""
    _fields_ = [("N", ctypes.c_int), ("C", ctypes.c_int), ("K_obs", ctypes.c_int), ("K_nbr", ctypes.c_int),
                ("grav", ctypes.c_double), ("hcom", ctypes.c_double), ("Ts", ctypes.c_double), ("mu", ctypes.c_double),
                ("Qw", ctypes.c_double), ("Pw", ctypes.c_double), ("Rw", ctypes.c_double), ("Sw", ctypes.c_double),
                ("box", ctypes.c_double), ("eps_obs", ctypes.c_double), ("eps_nbr", ctypes.c_double),
                ("vsat", ctypes.c_double), ("tol", ctypes.c_double),
                ("qp_maxit", ctypes.c_int), ("nlp_maxit", ctypes.c_int), ("use_nlp", ctypes.c_int)]

    @property
    def nv(self) -> int:
        return (6 + self.C) * self.N + 1

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Batch(ctypes.Structure):
    """Mirror of srb_batch (struct_size is filled in by the constructor)."""
    _fields_ = [("struct_size", ctypes.c_int), ("x0", _dp), ("ref", _dp), ("foot", _dp), ("obstacles", _dp), ("nbr_state", _dp),
                ("n_obs", ctypes.c_int), ("n_all", ctypes.c_int), ("agent_offset", ctypes.c_int),
                ("x_qp", _dp), ("x", _dp), ("obj", _dp), ("status", _ip), ("iters", _ip),
                ("alpha_buf", _dp), ("alpha", _dp), ("sel", _ip), ("obstacles_version", ctypes.c_int),
                ("nbr_plan", _dp), ("plan", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Batch), *args, **kw)


class Prep(ctypes.Structure):
    """Mirror of srb_prep (input assembly on the device; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("Pr", _dp), ("Prd", _dp), ("n_rows", ctypes.c_int), ("T", ctypes.c_int), ("agent_offset", ctypes.c_int),
                ("agent_id", _ip), ("gait_domain", _ip), ("contact", _ip),
                ("toe", _dp), ("start", _dp), ("q", _dp), ("dq", _dp),
                ("x0", _dp), ("ref", _dp), ("foot", _dp), ("last_state", _dp), ("status", _ip)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Prep), *args, **kw)


class Sim(ctypes.Structure):
    """Mirror of srb_sim (the closed-loop rollout; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("state", _dp), ("goal", _dp), ("phase", _ip), ("vref", ctypes.c_double),
                ("c_first", ctypes.c_int), ("x", _dp), ("status", _ip), ("iters", _ip),
                ("x0", _dp), ("ref", _dp), ("foot", _dp), ("last_state", _dp), ("alpha_buf", _dp), ("plan_table", _dp),
                ("traj", _dp), ("status_log", _ip), ("iters_log", _ip), ("x_log", _dp),
                ("obstacles", _dp), ("nbr_state", _dp),
                ("n_obs", ctypes.c_int), ("n_all", ctypes.c_int), ("agent_offset", ctypes.c_int),
                ("d_obs", _dp), ("d_agent", _dp), ("min_d_obs", _dp), ("min_d_agent", _dp), ("fail_cycle", _ip),
                ("distance_to_fail", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Sim), *args, **kw)


class Moving(ctypes.Structure):
    """Mirror of srb_moving (moving obstacles; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("obs_vel", _dp), ("horizon_selection", ctypes.c_int), ("obstacles", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Moving), *args, **kw)


class Sizes(ctypes.Structure):
    """Mirror of srb_sizes (obstacle sizes; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("obs_eps", _dp), ("obs_radius", _dp), ("clearance_selection", ctypes.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Sizes), *args, **kw)


class AgentSizes(ctypes.Structure):
    """Mirror of srb_agent_sizes (agent sizes; struct_size filled in)."""
    _fields_ = [("struct_size", ctypes.c_int), ("agent_rad", _dp), ("agent_pad", _dp), ("agent_body", _dp),
                ("clearance_selection", ctypes.c_int), ("collide_cycle", _ip)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(AgentSizes), *args, **kw)


class Plant(ctypes.Structure):
    """Mirror of srb_plant (the disturbed plant of the LIP rollout; struct_size filled in).  The SRB-12 mode's is
    srb12.PlantStruct12, filled from a srb12.Plant12."""
    _fields_ = [("struct_size", ctypes.c_int), ("seed", ctypes.c_ulonglong), ("kick_v", _dp), ("kick_p", _dp),
                ("plant_hcom", _dp), ("n_push", ctypes.c_int), ("push_cycle", _ip), ("push_agent", _ip), ("push_dv", _dp),
                ("dist_log", _dp)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Plant), *args, **kw)


class Link(ctypes.Structure):
    """Mirror of srb_link (the degraded neighbour link of a rollout, both modes; struct_size filled in).  A Rollout or
    srb12.Rollout12 fills it from a LinkModel and buffers of its own."""
    _fields_ = [("struct_size", ctypes.c_int), ("seed", ctypes.c_ulonglong), ("delay", _ip), ("drop", _dp),
                ("noise_p", _dp), ("noise_v", _dp), ("max_delay", ctypes.c_int), ("extrapolate", ctypes.c_int),
                ("ring_state", _dp), ("ring_plan", _dp), ("held_state", _dp), ("held_plan", _dp), ("held_cycle", _ip),
                ("seen_state", _dp), ("seen_plan", _dp), ("age_log", _ip)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(Link), *args, **kw)


class LinkModel:
    """What degrades the neighbour link of a Rollout or a srb12.Rollout12 (Rollout(link=LinkModel(...)); srb_link of
    include/srbnmpc.h): one broadcast per agent per cycle, and every receiver sees the same fate of it.

    seed      the key of the loss and noise draws (0 .. 2^64 - 1; Philox4x32-10, counters (cycle, global row, 2 / 3, 0):
              the plant's kicks use other counters, so one seed may serve both)
    delay     [n_all] int32 or None: cycles a row's messages are late, 0 .. 16
    drop      [n_all] float64 or None: the probability that a message of the row is lost, 0 .. 1
    noise_p, noise_v  [n_all] float64 or None: the bound (m, m/s) of the uniform error on the sent position / velocity
    extrapolate  True: the receivers dead-reckon a held message by its age (position along the held velocity, the
              held plan shifted by 4 grids per cycle of age); False: they use it as it is
    The tables are torch tensors on the rollout's device (checked there, by name) and do not change over a rollout; every
    shard holds them whole.  With every table None the link degrades nothing and the rollout is the plain one."""

    def __init__(self, seed: int = 0, delay=None, drop=None, noise_p=None, noise_v=None, extrapolate: bool = False):
        self.seed, self.delay, self.drop, self.noise_p, self.noise_v = seed, delay, drop, noise_p, noise_v
        self.extrapolate = extrapolate

    @property
    def on(self) -> bool:
        return any(t is not None for t in (self.delay, self.drop, self.noise_p, self.noise_v))


_lib = None


def use_library(name: str):
    """Diagnostics only: load the variant build `name` (libsrbnmpc_<tag>.so in this package
    directory) instead of the product library.  Must precede the first load."""
    global LIB_PATH
    base = os.path.basename(name)
    if base != name or not (base == "libsrbnmpc.so" or (base.startswith("libsrbnmpc_") and base.endswith(".so"))):
        raise ValueError(f"srbnmpc.use_library: expected libsrbnmpc.so or libsrbnmpc_<tag>.so, got {name!r}")
    path = os.path.join(_HERE, base)
    if _lib is not None and path != LIB_PATH:
        raise RuntimeError(f"srbnmpc.use_library: {LIB_PATH} is already loaded")
    LIB_PATH = path


def lib():
    """Load libsrbnmpc.so; raise loudly when it is missing (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"srbnmpc: {LIB_PATH} not built (run __graft_entry__.build() or make -C srb-cbf-nmpc_amd)")
        L = ctypes.CDLL(LIB_PATH)
        L.srb_params_default.argtypes = [ctypes.POINTER(Params), ctypes.c_int, ctypes.c_int]
        L.srb_nv.argtypes = [ctypes.POINTER(Params)]
        L.srb_lds_bytes.argtypes = [ctypes.POINTER(Params)]
        L.srb_ctx_create.argtypes = [ctypes.POINTER(Params), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.srb_ctx_destroy.argtypes = [ctypes.c_void_p]
        for f in ("srb_solve_batch", "srb_solve_qp"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch)]
        L.srb_solve_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.c_void_p]
        L.srb_select_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.c_int, ctypes.c_void_p]
        L.srb_sync.argtypes = [ctypes.c_void_p]
        L.srb_ctx_set_waves.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.srb_ctx_waves.argtypes = [ctypes.c_void_p]
        _cpp = ctypes.POINTER(ctypes.c_char_p)
        L.srb_ctx_last_kernels.argtypes = [ctypes.c_void_p, _cpp, _cpp]
        L.srb_kernel_table.argtypes = [ctypes.c_int, _ip, _cpp]
        L.srb_pick_kernel.argtypes = [ctypes.POINTER(Params), ctypes.c_int, _ip]
        L.srb_check_params.argtypes = [ctypes.POINTER(Params)]
        L.srb_ctx_set_scenes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.srb_ctx_scenes.argtypes = [ctypes.c_void_p, _ip, _ip]
        L.srb_ctx_set_qp_init.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.srb_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        L.srb_ctx_get_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.srb_last_polish_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        L.srb_hl_plan.argtypes = [ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp]
        L.srb_prepare_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Prep), ctypes.c_void_p]
        for f in ("srb_sim_advance_device", "srb_sim_metrics_device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Sim), ctypes.c_int, ctypes.c_void_p]
        L.srb_rollout_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim),
                                         ctypes.c_int, ctypes.c_void_p]
        L.srb_solve_batch_moving.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Moving)]
        L.srb_solve_batch_moving_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch),
                                                    ctypes.POINTER(Moving), ctypes.c_void_p]
        L.srb_select_moving_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Moving),
                                               ctypes.c_int, ctypes.c_void_p]
        L.srb_obstacles_advance_device.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, _dp, ctypes.c_void_p]
        L.srb_rollout_moving_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim),
                                                ctypes.POINTER(Moving), ctypes.c_int, ctypes.c_void_p]
        MV, SZ = ctypes.POINTER(Moving), ctypes.POINTER(Sizes)
        L.srb_solve_batch_sized.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ]
        L.srb_solve_batch_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ, ctypes.c_void_p]
        L.srb_select_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ, ctypes.c_int,
                                              ctypes.c_void_p]
        L.srb_sim_metrics_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Sim), SZ, ctypes.c_int,
                                                   ctypes.c_void_p]
        L.srb_rollout_sized_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim), MV,
                                               SZ, ctypes.c_int, ctypes.c_void_p]
        AG = ctypes.POINTER(AgentSizes)
        L.srb_solve_batch_agents.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ, AG]
        L.srb_solve_batch_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ, AG,
                                                    ctypes.c_void_p]
        L.srb_select_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), MV, SZ, AG, ctypes.c_int,
                                               ctypes.c_void_p]
        L.srb_sim_metrics_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Sim), SZ, AG, ctypes.c_int,
                                                    ctypes.c_void_p]
        L.srb_rollout_agents_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim), MV,
                                                SZ, AG, ctypes.c_int, ctypes.c_void_p]
        PL = ctypes.POINTER(Plant)
        L.srb_sim_advance_plant_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Sim), PL, ctypes.c_int,
                                                   ctypes.c_void_p]
        L.srb_rollout_plant_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim), MV,
                                               SZ, AG, PL, ctypes.c_int, ctypes.c_void_p]
        LN = ctypes.POINTER(Link)
        L.srb_link_update_device.argtypes = [ctypes.c_void_p, ctypes.c_int, LN, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p]
        L.srb_link_update_lanes_device.argtypes = [ctypes.c_void_p, ctypes.c_int, LN, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p]
        L.srb_rollout_link_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Batch), ctypes.POINTER(Sim), MV,
                                              SZ, AG, PL, LN, ctypes.c_int, ctypes.c_void_p]
        L.srb_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.srb_fit_bezier.argtypes = [_dp, _dp, _dp]
        L.srb_last_error.restype = ctypes.c_char_p
        if L.srb_abi_version() != ABI_VERSION:
            raise RuntimeError(f"srbnmpc: {LIB_PATH} has ABI {L.srb_abi_version()}, these bindings {ABI_VERSION} (rebuild)")
        _lib = L
    return _lib


def default_params(N: int = 4, C: int = 4, **overrides) -> Params:
    p = Params()
    lib().srb_params_default(ctypes.byref(p), N, C)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def lds_bytes(p: Params) -> int:
    return lib().srb_lds_bytes(ctypes.byref(p))


def check_params(p: Params) -> bool:
    """True where srb_ctx_create would accept p (srb_check_params; no device needed)."""
    return lib().srb_check_params(ctypes.byref(p)) == 0


def kernel_table():
    """The shipped solve-kernel instances (srb_kernel_table; no device needed): a list of
    ((NZL, TS, NW, NC, CC, KC), solve kernel name), the fp32-factor entries after the fp64 ones."""
    out = []
    while True:
        d = (ctypes.c_int * 6)(); name = ctypes.c_char_p()
        if lib().srb_kernel_table(len(out), d, ctypes.byref(name)) != 0:
            return out
        out.append((tuple(d), name.value.decode()))


def pick_kernel(p: Params, waves: int):
    """(NZL, TS, NW, NC, CC, KC) of the fp64 instance a launch of problem p wanting `waves` waves per agent picks
    with 160 KiB of LDS (srb_pick_kernel; no device needed); raises where no instance fits."""
    d = (ctypes.c_int * 6)()
    _check(lib().srb_pick_kernel(ctypes.byref(p), int(waves), d))
    return tuple(d)


def _check(rc: int):
    if rc != 0:
        raise RuntimeError(f"srbnmpc error {rc}: {lib().srb_last_error().decode()}")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    if a is None:
        return None
    if a.dtype == np.float64:
        return a.ctypes.data_as(_dp)
    return a.ctypes.data_as(_ip)


def _dptr(t):
    """A device tensor's address as double * (None stays None: the C ABI's "absent"); _p for torch tensors."""
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), _dp)


def _iptr(t):
    return None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), _ip)


def _clamp_selected(K_obs: int, K_nbr: int, n_obs: int, n_all: int, scenes):
    """(Ko, Kn) of "up to K nearest" for tables of these sizes, as the C ABI clamps them: to the tables, or with a
    scene partition (scene_agents, scene_obs) to the agent's own sub-tables."""
    rows, others = max(n_obs, 0), max(n_all - 1, 0)
    if scenes[0] > 0:
        rows, others = min(rows, scenes[1]), (scenes[0] - 1 if n_all > 0 else 0)
    return min(K_obs, rows), min(K_nbr, others)


def _moving_args(obs_vel, obs_horizon, n_obs, dtype, ptr, obstacle_rows=True) -> Moving:
    """The srb_moving of a solve / select call, both modes, after the checks of obs_vel that need no context, by name
    (obs_horizon without obs_vel is the library's refusal).  ptr: _p for host arrays, _dptr for device tensors."""
    if not obstacle_rows:
        raise ValueError("obs_vel / obs_horizon: the QP-only solve has no obstacle rows")
    if obs_vel is not None:
        _check_vel_array(obs_vel, n_obs, dtype)
    return Moving(ptr(obs_vel), int(bool(obs_horizon)), None)


def _sizes_args(obs_eps, obs_radius, obs_clearance, n_obs, dtype, ptr, obstacle_rows=True, device=None) -> Sizes:
    """The srb_sizes of a call after the checks of the tables that need no context, by name (obs_clearance without
    obs_eps is the library's refusal).  ptr: _p for host arrays, _dptr for device tensors."""
    if not obstacle_rows:
        raise ValueError("obs_eps / obs_clearance: the QP-only solve has no obstacle rows")
    if obs_eps is not None:
        _check_size_array(obs_eps, n_obs, dtype, "obs_eps", device)
    if obs_radius is not None:
        _check_size_array(obs_radius, n_obs, dtype, "obs_radius", device)
    return Sizes(ptr(obs_eps), ptr(obs_radius), int(bool(obs_clearance)))


def _agent_args(agent_rad, agent_pad, agent_body, nbr_clearance, n_all, dtype, ptr, obstacle_rows=True, device=None,
                checked=None) -> AgentSizes:
    """The srb_agent_sizes of a call after the checks of the tables that need no context, by name (nbr_clearance
    without agent_rad is the library's refusal).  ptr: _p for host arrays, _dptr for device tensors; checked: a
    solver's record of the device tensors whose values it has looked at (_check_agent_array)."""
    if not obstacle_rows:
        raise ValueError("agent_rad / agent_pad / nbr_clearance: the QP-only solve has no obstacle rows")
    for name, tab in (("agent_rad", agent_rad), ("agent_pad", agent_pad), ("agent_body", agent_body)):
        if tab is not None:
            _check_agent_array(tab, n_all, dtype, name, device, checked)
    return AgentSizes(ptr(agent_rad), ptr(agent_pad), ptr(agent_body), int(bool(nbr_clearance)), None)


class _SolverBase:
    """What BatchSolver and srb12.Solver12 share: the context's life, the stream of a launch, the scene partition,
    the record of the validated agent-size tensors and the Jacobi loop of solve_coupled_device.  A mode names the prefix of its entry points (_abi) and, where
    they are bound on first use, the function that loads the library (_lib)."""
    _abi = "srb"
    _lib = staticmethod(lib)

    def __init__(self, params, max_agents: int, device: int = 0):
        self.params = params
        self.max_agents = int(max_agents)
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(self._entry("ctx_create")(ctypes.byref(params), self.max_agents, self.device, ctypes.byref(h)))
        self._h = h
        self._scenes = (0, 0)

    def _entry(self, name: str):
        return getattr(self._lib(), f"{self._abi}_{name}")

    def _agent_checked(self) -> set:
        """The agent-size tensors whose values this solver has validated (looking at a device tensor's values
        synchronises with the host: once per tensor and version, not once per solve)."""
        if not hasattr(self, "_agent_ok"):
            self._agent_ok = set()
        return self._agent_ok

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._entry("ctx_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream):
        """hipStream_t for a launch: the caller's, else torch's current stream on this device
        (the C ABI's NULL would mean the context's own stream, unordered against torch's)."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
        return ctypes.c_void_p(stream)

    def set_scenes(self, scene_agents: int = 0, scene_obs: int = 0):
        """The batch as independent teams (srb_ctx_set_scenes / srb12_ctx_set_scenes): scene_agents agents and
        scene_obs obstacle rows per scene, tables flat and scene-major; agent g selects and is measured within scene
        g // scene_agents, sel holds global rows.  (0, 0): off, one team."""
        _check(self._entry("ctx_set_scenes")(self._h, int(scene_agents), int(scene_obs)))
        a, o = ctypes.c_int(), ctypes.c_int()
        _check(self._entry("ctx_scenes")(self._h, ctypes.byref(a), ctypes.byref(o)))
        self._scenes = (a.value, o.value)

    @property
    def scenes(self):
        """(scene_agents, scene_obs) as last set through set_scenes; (0, 0) when off."""
        return self._scenes

    def _solve_coupled(self, args, outer, exchange, nbr_plan, agent_offset, stream, round_kw, **kw):
        """The Jacobi loop of solve_coupled_device.  args: the mode's positional arguments of solve_device (x0 first,
        nbr_state and out last); round_kw(table): the mode's own keywords for the round that solves against `table`;
        kw: the keywords every round gets."""
        import torch
        x0, nbr_state, out = args[0], args[-2], args[-1]
        outer = int(outer)
        if outer < 1:
            raise ValueError("outer must be >= 1")
        plan = out.get("plan")
        if plan is None:
            raise ValueError("solve_coupled_device needs out['plan'] ([A][N][2] float64)")
        A, N = x0.shape[0], self.params.N
        _check_plan_array(plan, (A, N, 2), "out['plan']", torch.float64)
        if exchange is None and outer > 1 and (nbr_state is None or nbr_state.shape[0] != A or agent_offset != 0):
            raise ValueError("solve_coupled_device without an exchange iterates over this batch's own plans: "
                             "nbr_state must hold exactly the batch's agents (agent_offset 0)")
        other = getattr(self, "_plan_pong", None)
        if outer > 1 and (other is None or other.shape != plan.shape or other.device != plan.device):
            other = self._plan_pong = torch.empty_like(plan)
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream)) if stream is not None else contextlib.nullcontext()
        change = torch.zeros(max(outer - 1, 0), dtype=torch.float64, device=plan.device)
        with ctx:
            table, prev = nbr_plan, None
            for r in range(outer):
                cur = plan if (outer - 1 - r) % 2 == 0 else other      # the last round writes out["plan"]
                if r > 0:
                    table = exchange(prev) if exchange is not None else prev
                self.solve_device(*args, agent_offset=agent_offset, stream=stream, nbr_plan=table, plan=cur,
                                  **round_kw(table), **kw)
                if r > 0:
                    change[r - 1] = (cur - prev).abs().max()
                prev = cur
        return change


class BatchSolver(_SolverBase):
    """One HIP context solving batches of up to `max_agents` agents.

    solve(...)        host numpy in/out (srb_solve_batch, synchronous)
    solve_device(...) torch CUDA tensors in/out (srb_solve_batch_device, async on a stream)
    """

    # --------------------------------------------------------------- host path
    def n_selected(self, n_obs: int, n_all: int):
        """(Ko, Kn): selected static obstacles / neighbours per agent for tables of these sizes
        ("up to K nearest", the clamp the C ABI applies)."""
        return _clamp_selected(self.params.K_obs, self.params.K_nbr, n_obs, n_all, self._scenes)

    def solve(self, x0, ref, foot, obstacles=None, nbr_state=None, agent_offset: int = 0, qp_only: bool = False,
              alpha_buf=None, nbr_plan=None, plan=None, obs_vel=None, obs_horizon: bool = False, obs_eps=None,
              obs_clearance: bool = False, agent_rad=None, agent_pad=None, nbr_clearance: bool = False):
        """Host arrays in, dict of outputs back.  alpha_buf ([A][4], the Bezier buffer state)
        additionally returns alpha ([A][4][5], get_alphaCOM) from the fused fit.  With the NLP
        stage, sel ([A][Ko + Kn]) holds the selected obstacle / neighbour rows.  nbr_plan
        ([n_all][N][2], float64, C-contiguous) makes the neighbour rows follow the neighbours' plans
        instead of the constant-velocity guess; plan ([A][N][2], the same) receives this batch's plans
        (out["plan"]; allocated here when None).  obs_vel ([n_obs][2], float64, C-contiguous): the obstacles move
        at these velocities over the horizon (srb_solve_batch_moving); obs_horizon=True additionally selects the
        static columns by closest predicted approach instead of nearest now.  obs_eps ([n_obs], float64, C-contiguous):
        the CBF level of each obstacle row in squared metres, the unit of eps_obs (srb_solve_batch_sized);
        obs_clearance=True additionally selects the static columns by clearance to the level set.  agent_rad, agent_pad
        ([n_all], float64, C-contiguous, finite; agent_rad >= 0): a safety radius and a pad per row of nbr_state
        (srb_solve_batch_agents): neighbour column j at the level (agent_rad[g] + agent_rad[sel[j]])^2, every static
        column of agent g at (sqrt(level) + agent_pad[g])^2; nbr_clearance=True additionally selects the neighbour
        columns by clearance dist - agent_rad."""
        p = self.params
        x0 = _f64(x0).reshape(-1, 4)
        A = x0.shape[0]
        ref = _f64(ref).reshape(A, 4 * p.N)
        foot = _f64(foot).reshape(A, p.N * 2 * p.C)
        ob = _f64(obstacles if obstacles is not None else np.zeros((0, 2))).reshape(-1, 2)
        nb = _f64(nbr_state).reshape(-1, 4) if nbr_state is not None else None
        out = dict(x_qp=np.zeros((A, p.nv)), x=np.zeros((A, p.nv)), obj=np.zeros(A),
                   status=np.zeros((A, 2), np.int32), iters=np.zeros((A, 2), np.int32))
        ab = None
        if alpha_buf is not None:
            ab = _f64(alpha_buf).reshape(A, 4)
            out["alpha"] = np.zeros((A, 4, 5))
        Ko, Kn = self.n_selected(ob.shape[0], nb.shape[0] if nb is not None else 0)
        out["sel"] = np.full((A, Ko + Kn), -2, np.int32)
        if nbr_plan is not None:
            # (without nbr_state the row count is the table's own: the library refuses that call by name)
            _check_plan_array(nbr_plan, (nb.shape[0] if nb is not None else len(nbr_plan), p.N, 2), "nbr_plan", np.float64)
        if plan is None:
            plan = np.zeros((A, p.N, 2))
        _check_plan_array(plan, (A, p.N, 2), "plan", np.float64)
        out["plan"] = plan
        b = Batch(_p(x0), _p(ref), _p(foot), _p(ob) if ob.size else None, _p(nb) if nb is not None else None,
                  ob.shape[0], nb.shape[0] if nb is not None else 0, int(agent_offset),
                  _p(out["x_qp"]), _p(out["x"]), _p(out["obj"]), _p(out["status"]), _p(out["iters"]),
                  _p(ab) if ab is not None else None, _p(out["alpha"]) if ab is not None else None,
                  _p(out["sel"]) if out["sel"].size and not qp_only else None, 0, _p(nbr_plan), _p(plan))
        moving = obs_vel is not None or obs_horizon
        mv = _moving_args(obs_vel, obs_horizon, ob.shape[0], np.float64, _p, not qp_only) if moving else None
        if agent_rad is not None or agent_pad is not None or nbr_clearance:
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, ob.shape[0], np.float64, _p, not qp_only) if sized else None
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, nb.shape[0] if nb is not None else 0, np.float64, _p,
                             not qp_only)
            _check(lib().srb_solve_batch_agents(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                                ctypes.byref(sz) if sized else None, ctypes.byref(ag)))
            return out
        if obs_eps is not None or obs_clearance:
            sz = _sizes_args(obs_eps, None, obs_clearance, ob.shape[0], np.float64, _p, not qp_only)
            _check(lib().srb_solve_batch_sized(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                               ctypes.byref(sz)))
            return out
        if moving:
            _check(lib().srb_solve_batch_moving(self._h, A, ctypes.byref(b), ctypes.byref(mv)))
            return out
        fn = lib().srb_solve_qp if qp_only else lib().srb_solve_batch
        _check(fn(self._h, A, ctypes.byref(b)))
        return out

    # --------------------------------------------------------------- device path
    def solve_device(self, x0, ref, foot, obstacles, nbr_state, out, agent_offset: int = 0, stream=None,
                     alpha_buf=None, obstacles_version: int = 0, nbr_plan=None, plan=None, obs_vel=None,
                     obs_horizon: bool = False, obs_eps=None, obs_clearance: bool = False, agent_rad=None, agent_pad=None,
                     nbr_clearance: bool = False):
        """All arguments torch tensors on this solver's device (float64 / int32), contiguous.
        `out` is a dict with x_qp (or None), x, obj, status, iters and, with alpha_buf [A][4],
        alpha [A][20]; an optional int32 out["sel"] [A][Ko + Kn] receives the selected rows
        (otherwise the context's scratch is used: one stream per context at a time).
        obstacles_version != 0 marks the obstacle tensor as unchanged since the last call with
        that version (its selection grid is reused; the reference's obstacles are static).
        nbr_plan ([n_all][N][2] float64, contiguous): the neighbours' plans for the inter-agent rows
        (None: constant velocity); plan (or out["plan"], [A][N][2] float64): receives this batch's plans,
        and must not overlap nbr_plan.  obs_vel ([n_obs][2] float64, contiguous): the obstacles' velocities
        (srb_solve_batch_moving_device; needs obstacles_version 0); obs_horizon=True selects the static columns by
        closest predicted approach over the horizon.  obs_eps ([n_obs] float64, contiguous): the CBF level of each
        obstacle row (srb_solve_batch_sized_device; goes together with obstacles_version); obs_clearance=True selects
        the static columns by clearance to the level set.  agent_rad, agent_pad ([n_all] float64, contiguous, finite;
        agent_rad >= 0): a safety radius and a pad per row of nbr_state (srb_solve_batch_agents_device; the values of
        a tensor are looked at once, on its first use with this solver); nbr_clearance=True selects the neighbour
        columns by clearance dist - agent_rad.
        Asynchronous on `stream` (a hipStream_t handle), by default torch's current stream on
        this device, so the launch is ordered after the torch work that filled the inputs."""
        A = x0.shape[0]
        Ko, Kn = self.n_selected(0 if obstacles is None else obstacles.shape[0],
                                 0 if nbr_state is None else nbr_state.shape[0])
        sel = out.get("sel")
        # the kernel writes rows of stride Ko + Kn (K clamped to the table sizes): the tensor must
        # have exactly that row length, or its rows would be read misaligned
        if sel is not None and (sel.dtype != torch_int32() or tuple(sel.shape) != (A, Ko + Kn) or not sel.is_contiguous()):
            raise ValueError(f"out['sel'] must be a contiguous int32 tensor of shape ({A}, {Ko + Kn}) "
                             f"(K_obs, K_nbr clamped to the table sizes: BatchSolver.n_selected), got "
                             f"{tuple(sel.shape)} {sel.dtype}")
        if plan is None:
            plan = out.get("plan")
        N = self.params.N
        if nbr_plan is not None:
            _check_plan_array(nbr_plan, (nbr_plan.shape[0] if nbr_state is None else nbr_state.shape[0], N, 2), "nbr_plan",
                              torch_float64())
        if plan is not None:
            _check_plan_array(plan, (A, N, 2), "plan", torch_float64())
        b = Batch(_dptr(x0), _dptr(ref), _dptr(foot), _dptr(obstacles), _dptr(nbr_state),
                  0 if obstacles is None else obstacles.shape[0], 0 if nbr_state is None else nbr_state.shape[0],
                  int(agent_offset), _dptr(out.get("x_qp")), _dptr(out["x"]), _dptr(out["obj"]),
                  _iptr(out["status"]), _iptr(out["iters"]), _dptr(alpha_buf),
                  _dptr(out.get("alpha") if alpha_buf is not None else None), _iptr(sel), int(obstacles_version),
                  _dptr(nbr_plan), _dptr(plan))
        n_obs = 0 if obstacles is None else obstacles.shape[0]
        moving = obs_vel is not None or obs_horizon
        mv = _moving_args(obs_vel, obs_horizon, n_obs, torch_float64(), _dptr) if moving else None
        if agent_rad is not None or agent_pad is not None or nbr_clearance:
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch_float64(), _dptr, device=x0.device) if sized else None
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, 0 if nbr_state is None else nbr_state.shape[0],
                             torch_float64(), _dptr, device=x0.device, checked=self._agent_checked())
            _check(lib().srb_solve_batch_agents_device(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                                       ctypes.byref(sz) if sized else None, ctypes.byref(ag),
                                                       self._stream(stream)))
            return
        if obs_eps is not None or obs_clearance:
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch_float64(), _dptr, device=x0.device)
            _check(lib().srb_solve_batch_sized_device(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                                      ctypes.byref(sz), self._stream(stream)))
            return
        if moving:
            _check(lib().srb_solve_batch_moving_device(self._h, A, ctypes.byref(b), ctypes.byref(mv), self._stream(stream)))
            return
        _check(lib().srb_solve_batch_device(self._h, A, ctypes.byref(b), self._stream(stream)))

    def select_device(self, x0, obstacles, nbr_state, sel, tables: int = 3, agent_offset: int = 0, stream=None,
                      obstacles_version: int = 0, nbr_plan=None, obs_vel=None, obs_horizon: bool = False, obs_eps=None,
                      obs_clearance: bool = False, agent_rad=None, agent_pad=None, nbr_clearance: bool = False):
        """The obstacle / neighbour selection alone (srb_select_device) into the int32 tensor sel [A][Ko + Kn]:
        tables 1 the static obstacles, 2 the neighbour snapshot, 3 both.  With the option "selection" set
        to 0, solve_device then uses out["sel"] as filled here (bench.py selects the static obstacles while
        the neighbour all-gather is in flight).  With the option "plan_selection" set to 1, tables & 2 is the
        horizon-aware selection (closest predicted approach) and needs nbr_plan [n_all][N][2].  With obs_vel
        ([n_obs][2]) and obs_horizon=True, tables & 1 is the horizon-aware obstacle selection
        (srb_select_moving_device).  With obs_eps ([n_obs]) and obs_clearance=True, tables & 1 is the selection by
        clearance to the level set (srb_select_sized_device), over the horizon when obs_horizon is on as well.
        With agent_rad ([n_all]) and nbr_clearance=True, tables & 2 is the neighbour selection by clearance
        dist - agent_rad (srb_select_agents_device), over the horizon with "plan_selection" and nbr_plan; agent_pad
        is validated and otherwise not read by a selection.
        Asynchronous on `stream` like solve_device."""
        A = x0.shape[0]
        Ko, Kn = self.n_selected(0 if obstacles is None else obstacles.shape[0],
                                 0 if nbr_state is None else nbr_state.shape[0])
        if sel.dtype != torch_int32() or tuple(sel.shape) != (A, Ko + Kn) or not sel.is_contiguous():
            raise ValueError(f"sel must be a contiguous int32 tensor of shape ({A}, {Ko + Kn}), got {tuple(sel.shape)} {sel.dtype}")
        if nbr_plan is not None:
            _check_plan_array(nbr_plan, (nbr_plan.shape[0] if nbr_state is None else nbr_state.shape[0], self.params.N, 2), "nbr_plan",
                              torch_float64())
        b = Batch(_dptr(x0), None, None, _dptr(obstacles), _dptr(nbr_state),
                  0 if obstacles is None else obstacles.shape[0], 0 if nbr_state is None else nbr_state.shape[0],
                  int(agent_offset), None, None, None, None, None, None, None,
                  _iptr(sel), int(obstacles_version), _dptr(nbr_plan), None)
        n_obs = 0 if obstacles is None else obstacles.shape[0]
        moving = obs_vel is not None or obs_horizon
        mv = _moving_args(obs_vel, obs_horizon, n_obs, torch_float64(), _dptr) if moving else None
        if agent_rad is not None or agent_pad is not None or nbr_clearance:
            sized = obs_eps is not None or obs_clearance
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch_float64(), _dptr, device=x0.device) if sized else None
            ag = _agent_args(agent_rad, agent_pad, None, nbr_clearance, 0 if nbr_state is None else nbr_state.shape[0],
                             torch_float64(), _dptr, device=x0.device, checked=self._agent_checked())
            _check(lib().srb_select_agents_device(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                                  ctypes.byref(sz) if sized else None, ctypes.byref(ag), int(tables),
                                                  self._stream(stream)))
            return
        if obs_eps is not None or obs_clearance:
            sz = _sizes_args(obs_eps, None, obs_clearance, n_obs, torch_float64(), _dptr, device=x0.device)
            _check(lib().srb_select_sized_device(self._h, A, ctypes.byref(b), ctypes.byref(mv) if moving else None,
                                                 ctypes.byref(sz), int(tables), self._stream(stream)))
            return
        if moving:
            _check(lib().srb_select_moving_device(self._h, A, ctypes.byref(b), ctypes.byref(mv), int(tables),
                                                  self._stream(stream)))
            return
        _check(lib().srb_select_device(self._h, A, ctypes.byref(b), int(tables), self._stream(stream)))

    def solve_coupled_device(self, x0, ref, foot, obstacles, nbr_state, out, outer: int = 2, exchange=None,
                             nbr_plan=None, agent_offset: int = 0, stream=None, alpha_buf=None,
                             obstacles_version: int = 0, obs_vel=None, obs_horizon: bool = False, obs_eps=None,
                             obs_clearance: bool = False, agent_rad=None, agent_pad=None, nbr_clearance: bool = False):
        """Jacobi iteration over the agents' plans: `outer` solves of the same cycle, each against the plans
        the agents wrote in the round before.  Round 0 solves against nbr_plan (None: the constant-velocity
        rows); every later round r exchanges the plans of round r - 1 -- table = exchange(plan), a
        dist.PlanExchange, or on one GPU (exchange None: the batch is the whole team, agent_offset 0) the plan
        tensor itself -- and solves again.  The plans ping-pong between out["plan"] ([A][N][2], required) and
        a second buffer of this solver, so the table a round reads is never the buffer it writes; the last
        round's results, its plans included, are in `out`.  Returns plan_change, a device tensor [outer - 1]:
        max |plan_r - plan_{r-1}| per round (torch reductions; nothing synchronises with the host inside the
        loop).  No damping and no convergence test: the plain Jacobi round.  Other arguments (obs_vel,
        obs_horizon, obs_eps, obs_clearance, agent_rad, agent_pad and nbr_clearance included: every round solves
        against the same obstacle and agent tables) as solve_device."""
        return self._solve_coupled((x0, ref, foot, obstacles, nbr_state, out), outer, exchange, nbr_plan, agent_offset,
                                   stream, lambda table: {"alpha_buf": alpha_buf}, obstacles_version=obstacles_version,
                                   obs_vel=obs_vel, obs_horizon=obs_horizon, obs_eps=obs_eps, obs_clearance=obs_clearance,
                                   agent_rad=agent_rad, agent_pad=agent_pad, nbr_clearance=nbr_clearance)

    def prepare_device(self, Pr, Prd, gait_domain, contact, toe, start, q, dq, out, agent_id=None,
                       agent_offset: int = 0, stream=None):
        """Input assembly on the device (srb_prepare_batch_device): torch tensors on this
        solver's device.  Pr, Prd: [T, 2*NA] (column-major 2*NA x T); gait_domain [A] int32;
        contact [A,4] int32; toe [A,3,4]; start [A,2]; q, dq [A,18].  `out` holds x0 [A,4],
        ref [A,4N], foot [A,N*2*C], last_state [A,4], status [A] int32.  Asynchronous."""
        A = q.shape[0]
        pr = Prep(_dptr(Pr), _dptr(Prd), Pr.shape[1], Pr.shape[0], int(agent_offset), _iptr(agent_id),
                  _iptr(gait_domain), _iptr(contact), _dptr(toe), _dptr(start), _dptr(q), _dptr(dq),
                  _dptr(out["x0"]), _dptr(out["ref"]), _dptr(out["foot"]), _dptr(out["last_state"]), _iptr(out["status"]))
        _check(lib().srb_prepare_batch_device(self._h, A, ctypes.byref(pr), self._stream(stream)))

    def advance_obstacles_device(self, obstacles, obs_vel, stream=None):
        """One control cycle (4 grids) of a moving obstacle table, in place (srb_obstacles_advance_device):
        obstacles[i] += obs_vel[i] * (Ts * 4).  Both [n_obs][2] float64 tensors on this solver's device."""
        _check_vel_array(obstacles, obstacles.shape[0], torch_float64(), "obstacles")
        _check_vel_array(obs_vel, obstacles.shape[0], torch_float64())
        _check(lib().srb_obstacles_advance_device(self._h, obstacles.shape[0], _dptr(obstacles), _dptr(obs_vel),
                                                  self._stream(stream)))

    def sync(self):
        _check(lib().srb_sync(self._h))

    def set_waves(self, nw: int = 0):
        """Waves per agent (0 automatic, 1, 2, 4; srb_ctx_set_waves)."""
        _check(lib().srb_ctx_set_waves(self._h, int(nw)))

    def set_option(self, name: str, value: float):
        """Context option (srb_ctx_set_option): name one of OPTIONS ("polish", "polish_rho",
        "polish_waves", "grid_min_rows", "grid_min_rows_static", "polish_fused", "plan_selection", ..;
        "last_polish" is read only)."""
        _check(lib().srb_ctx_set_option(self._h, OPTIONS[name], float(value)))

    def get_option(self, name: str) -> float:
        v = ctypes.c_double()
        _check(lib().srb_ctx_get_option(self._h, OPTIONS[name], ctypes.byref(v)))
        return v.value

    def polish_fused_active(self) -> bool:
        """True when the last launch ran the polish inside the solve kernel (SRB_OPT_LAST_POLISH = 2)."""
        return self.get_option("last_polish") == 2.0

    def set_qp_init(self, mode: int = 1):
        """QP-stage starting point (srb_ctx_set_qp_init): 1 scaled (default), 0 iSWIFT's kkt_initialize."""
        _check(lib().srb_ctx_set_qp_init(self._h, int(mode)))

    def waves(self) -> int:
        """Waves per agent of the last launch."""
        return lib().srb_ctx_waves(self._h)

    def last_kernels(self):
        """(solve, polish): names of the kernels the last launch ran (srb_ctx_last_kernels); polish is "" where
        the polish ran fused into the solve kernel or not at all."""
        a = ctypes.c_char_p(); b = ctypes.c_char_p()
        _check(lib().srb_ctx_last_kernels(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value.decode(), b.value.decode()

    def last_kernel_ms(self):
        a = ctypes.c_float(); b = ctypes.c_float()
        _check(lib().srb_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def last_polish_ms(self) -> float:
        """HIP-event time of the last launch's polish kernel (srb_polish_kernel), ms (0 when fused)."""
        t = ctypes.c_float()
        _check(lib().srb_last_polish_ms(self._h, ctypes.byref(t)))
        return t.value


def torch_int32():
    import torch
    return torch.int32


def torch_float64():
    import torch
    return torch.float64


def _check_plan_array(a, shape, name, dtype):
    """Shape, dtype and contiguity of a plan array (numpy on the host path, torch on the device path), as
    out['sel'] is checked: the library reads rows of exactly this layout."""
    contiguous = a.is_contiguous() if hasattr(a, "is_contiguous") else a.flags["C_CONTIGUOUS"]
    if a.dtype != dtype or tuple(a.shape) != tuple(shape) or not contiguous:
        raise ValueError(f"{name} must be a contiguous float64 array of shape {tuple(shape)}, got "
                         f"{tuple(a.shape)} {a.dtype}")


def _check_vel_array(a, n_obs, dtype, name="obs_vel"):
    """obs_vel (or the table it belongs to): a contiguous float64 [n_obs][2] array, validated as nbr_plan is."""
    if not hasattr(a, "dtype") or not hasattr(a, "shape"):
        raise ValueError(f"{name} must be a contiguous float64 array of shape ({n_obs}, 2), got {type(a).__name__}")
    _check_plan_array(a, (n_obs, 2), name, dtype)


def _check_size_array(a, n_obs, dtype, name, device=None):
    """obs_eps / obs_radius: a contiguous float64 [n_obs] array (on `device` when one is given), by name."""
    if not hasattr(a, "dtype") or not hasattr(a, "shape"):
        raise ValueError(f"{name} must be a contiguous float64 array of shape ({n_obs},), got {type(a).__name__}")
    _check_plan_array(a, (n_obs,), name, dtype)
    if device is not None and getattr(a, "device", device) != device:
        raise ValueError(f"{name} must be on {device}, got {a.device}")


def _check_agent_array(a, n_all, dtype, name, device=None, checked=None):
    """agent_rad / agent_pad / agent_body: a contiguous float64 [n_all] array (on `device` when one is given) of
    finite values, agent_rad and agent_body not negative, by name.  checked: a set of the device tensors already
    looked at (data pointer, version, name), so a tensor used every cycle costs one host synchronisation."""
    _check_size_array(a, n_all, dtype, name, device)
    key = (a.data_ptr(), a._version, name, n_all) if hasattr(a, "data_ptr") and hasattr(a, "_version") else None
    if key is not None and checked is not None and key in checked:
        return
    if hasattr(a, "isfinite"):
        finite, neg = bool(a.isfinite().all()), bool((a < 0).any())
    else:
        finite, neg = bool(np.isfinite(a).all()), bool((a < 0).any())
    if not finite:
        raise ValueError(f"{name} must be finite (a NaN or infinite radius)")
    if name != "agent_pad" and neg:
        raise ValueError(f"{name} must be >= 0 (a radius in metres)")
    if key is not None and checked is not None:
        checked.add(key)


def hl_plan(Pstart, Pobs, loop: int = 100000, device: int = 0):
    """HL reference planner on the GPU (generateReferenceTrajectory, MPC_dist.cpp:930-1104).
    Pstart [NA, 2] (or flat 2NA), Pobs [n_obs, 2].  Returns Pr, Prd as (2NA, loop // 40)."""
    Ps = _f64(Pstart).reshape(-1)
    NA = Ps.size // 2
    ob = _f64(Pobs).reshape(-1, 2)
    T = int(loop) // 40
    Pr = np.zeros((T, 2 * NA)); Prd = np.zeros((T, 2 * NA))
    _check(lib().srb_hl_plan(int(device), NA, _p(Ps), _p(ob) if ob.size else None, ob.shape[0], int(loop),
                             _p(Pr), _p(Prd)))
    return Pr.T.copy(), Prd.T.copy()


def fit_bezier(buf, X):
    """fitComTrajectory_eventbase (MPC_dist.cpp:784-855): alpha_COM (4x5)."""
    a = np.zeros(20)
    lib().srb_fit_bezier(_p(_f64(buf)), _p(_f64(X)), _p(a))
    return a.reshape(4, 5)


def split(params: Params, x):
    """Split decision vectors (..., nv) into X (...,N,4), U (...,N,2), lambda (...,N,C), s (...)."""
    N, C = params.N, params.C
    x = np.asarray(x)
    return (x[..., :4 * N].reshape(*x.shape[:-1], N, 4), x[..., 4 * N:6 * N].reshape(*x.shape[:-1], N, 2),
            x[..., 6 * N:6 * N + C * N].reshape(*x.shape[:-1], N, C), x[..., -1])


from .mpc_dist import MPCDist  # noqa: E402
from . import workload  # noqa: E402
from . import ll_workload  # noqa: E402
from .lowlevel import LowLevelCtrl  # noqa: E402
from .rollout import Rollout  # noqa: E402
