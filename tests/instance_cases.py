"""Cases of the per-instance GPU matrices (tests/test_gpu_instances.py, tests/test_instances12_gpu.py): for every
shipped kernel instance the shapes that launch it, the batches and the oracle's answers, computed once and shared
(read only).  The shapes are the instance's smallest and its edges (a full slot trip, one slot over a trip, nz = NZL,
64 NW TS slots); which instance a shape lands on is not argued here but asserted by the tests through
BatchSolver.last_kernels() / Solver12.last_kernel().

Batches are workload.make_batch / make_batch12 with the seed of SEEDS / SEEDS12: chosen on the CPU so that, on the
oracle alone, at least half of the agents end NLP OPTIMAL and none ends KKTFAIL (oracle_is_fit, which every test
asserts), for the plain answer and for the moving-obstacle answer of the same batch.
"""
import numpy as np

import moving12_oracle
import moving_oracle
import oracle
import plan_oracle
from srbnmpc import workload

# ---------------------------------------------------------------------------- LIP mode
# (NZL, TS, NW): [(N, C, K), ..]; K_obs = min(K, 16), K_nbr = K - K_obs; the run-time instances (NC = CC = KC = 0)
LIP_RUN_TIME = {
    (8, 1, 1): [(5, 2, 1)],                            # 64 slots: a full trip
    (16, 1, 1): [(3, 4, 7)],                           # 62 slots, nz 10
    (12, 3, 1): [(3, 2, 10), (11, 2, 0)],              # 65 slots: one over a trip; nz = NZL
    (12, 4, 1): [(11, 2, 6)],                          # nz = NZL, 197 slots
    (16, 4, 1): [(4, 4, 3), (5, 4, 0)],                # nz 13; nz = 16
    (24, 5, 1): [(6, 4, 0), (23, 2, 0)],               # nz 19; nz = 24
    (24, 8, 1): [(23, 2, 2), (19, 2, 15)],             # nz = 24, 321 slots; 512 slots: full
    (32, 4, 1): [(8, 4, 0), (10, 4, 11)],              # nz 25; nz 31, 249 slots
    (32, 8, 1): [(10, 4, 12), (31, 2, 0), (27, 2, 7)],  # 259 slots; nz = 32; 512 slots
    (8, 1, 4): [(7, 2, 0)],                            # nz = 8
    (12, 1, 4): [(11, 2, 0)],
    (16, 1, 4): [(5, 4, 0)],
    (16, 2, 4): [(15, 2, 6)],                          # nz = 16, 269 slots
    (24, 2, 4): [(23, 2, 0), (19, 2, 15)],             # nz = 24; 512 slots
    (32, 2, 4): [(31, 2, 0), (27, 2, 7)],              # nz = 32; 512 slots
    (12, 2, 2): [(11, 2, 0)],
    (16, 2, 2): [(5, 4, 0)],
    (24, 4, 2): [(23, 2, 0), (19, 2, 15)],
}
# the compiled instances: dims and the one shape each is compiled for
LIP_COMPILED = [(12, 4, 1, 10, 2, 11), (12, 1, 4, 10, 2, 3), (24, 4, 2, 20, 2, 11)]
LIP_F32 = [(12, 4, 1, 10, 2, 11), (24, 4, 2, 20, 2, 11)]

# seed of workload.make_batch per shape (N, C, K); shapes not listed take DEFAULT_SEED
DEFAULT_SEED = 3
SEEDS = {}


def lip_cases():
    """[(dims, (N, C, K))]: every instance with each of its shapes."""
    out = [((nzl, ts, nw, 0, 0, 0), sh) for (nzl, ts, nw), shapes in LIP_RUN_TIME.items() for sh in shapes]
    return out + [(d, d[3:]) for d in LIP_COMPILED]


def tabled_shape(shape):
    """The shape a case's tabled form runs at: its own, except that K = 0 becomes K = 1 -- without an obstacle or
    neighbour column no table is read and the host launches the plain kernels."""
    N, C, K = shape
    return (N, C, max(K, 1))


def split_K(K):
    return min(K, 16), max(K - 16, 0)


def agents(K):
    return max(8, split_K(K)[1] + 1)


def slots(N, C, K):
    return (6 + C) * N + 1 + 2 * (N - 1) + 2 * N + N * K


_cache = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def lip_batch(shape):
    if ("b", shape) not in _cache:
        N, C, K = shape
        _cache[("b", shape)] = _frozen(workload.make_batch(agents(K), N, C, seed=SEEDS.get(shape, DEFAULT_SEED)))
    return _cache[("b", shape)]


def lip_params(shape):
    N, C, K = shape
    Ko, Kn = split_K(K)
    return oracle.params(N, C, K_obs=Ko, K_nbr=Kn)


def lip_velocities(shape):
    b = lip_batch(shape)
    return workload.obstacle_velocities(b["obstacles"].shape[0], SEEDS.get(shape, DEFAULT_SEED), 1.0)


def lip_plain(shape):
    """oracle.solve_batch of the shape's batch, with the oracle's selection as `sel`."""
    if ("r", shape) not in _cache:
        b, p = lip_batch(shape), lip_params(shape)
        r = oracle.solve_batch(p, b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nthreads=8)
        q = plan_oracle.clamped(p, b["obstacles"].shape[0], b["nbr_state"].shape[0])
        assert (q.K_obs, q.K_nbr) == (p.K_obs, p.K_nbr)            # neither K is clamped by the batch
        r["sel"] = np.array([oracle.select_idx(q, b["x0"][a], b["obstacles"], b["nbr_state"], a)
                             for a in range(b["x0"].shape[0])], np.int32).reshape(b["x0"].shape[0], p.K_obs + p.K_nbr)
        _cache[("r", shape)] = _frozen(r)
    return _cache[("r", shape)]


def lip_moving(shape):
    """moving_oracle.solve of the shape's batch against lip_velocities(shape)."""
    if ("m", shape) not in _cache:
        _cache[("m", shape)] = _frozen(moving_oracle.solve(lip_params(shape), lip_batch(shape), lip_velocities(shape)))
    return _cache[("m", shape)]


def oracle_is_fit(r):
    """The condition a case's batch meets on the oracle alone: at least half NLP OPTIMAL, none KKTFAIL."""
    st = np.asarray(r["status"])
    return (st[:, 1] == 0).mean() >= 0.5 and not (st == 1).any()


# ---------------------------------------------------------------------------- SRB-12 mode
# (N, K) at the trip edges: 4 N legs and N K obstacle rows over 64 lanes
SHAPES12 = [
    (16, 4),      # 4 N = 64 and N K = 64: both trips exactly full
    (17, 3),      # 68 legs: two leg trips
    (8, 8),
    (16, 8),      # 128 rows: two obstacle trips
    (16, 16),     # 256
    (16, 32),     # 512
    (20, 20),     # 400 rows with two leg trips
    (24, 32),     # 768 = 12 * 64: the largest shape there is
    (10, 11),     # compiled
    (20, 11),     # compiled
    (6, 0),       # no obstacle rows at all
]
DEFAULT_SEED12 = 31
SEEDS12 = {}


def batch12(shape):
    if ("b12", shape) not in _cache:
        N, K = shape
        _cache[("b12", shape)] = _frozen(workload.make_batch12(agents(K), N, "trot", seed=SEEDS12.get(shape, DEFAULT_SEED12)))
    return _cache[("b12", shape)]


def params12(shape):
    N, K = shape
    Ko, Kn = split_K(K)
    return oracle.params12(N, K_obs=Ko, K_nbr=Kn)


def velocities12(shape):
    b = batch12(shape)
    return workload.obstacle_velocities(b["obstacles"].shape[0], SEEDS12.get(shape, DEFAULT_SEED12), 1.0)


def plain12(shape):
    if ("r12", shape) not in _cache:
        b = batch12(shape)
        _cache[("r12", shape)] = _frozen(oracle.solve_batch12(params12(shape), b["x0"], b["xref"], b["foot"], b["contact"],
                                                              b["obstacles"], b["nbr_state"]))
    return _cache[("r12", shape)]


def moving12(shape):
    """K_nbr = 0 only (K <= 16): moving12_oracle.solve_moving, the oracle's own answer for the moving table."""
    assert split_K(shape[1])[1] == 0
    if ("m12", shape) not in _cache:
        b = batch12(shape)
        _cache[("m12", shape)] = _frozen(moving12_oracle.solve_moving(params12(shape), b, b["obstacles"], velocities12(shape)))
    return _cache[("m12", shape)]
