"""Cases that reach the NLP stage's inertia shift, selected from the oracle alone (tests/test_inertia_shift.py asserts
the selection on the CPU; tests/test_gpu_inertia_shift.py and tests/test_inertia12_gpu.py compare the kernels on them).

How the path is reached.  The curvature of the Lagrangian on (x_k, y_k) is Pd - 2 sum_j z_kj, and the obstacle duals of a
grid sum to about Sw * s.  Raising the slack weight Sw on a crowded batch (four times the reference's obstacle density)
makes the reduced Newton matrix indefinite for agents that stand inside an obstacle's level set: the factorisation fails
and the solver adds delta * Z'Z (LIP) / delta * I (SRB-12), delta = 1e-10 max(1, max diag), tenfold per further try.
At the default Sw the same batches never shift (asserted), so a case isolates the path.

The three sets of a case's agents, all from the oracle:
  shifted  at least one failed factorisation in the NLP loop (oracle.solve_batch(..., stats=True))
  strict   stable: status and iteration counts unchanged and X, U, s within STABLE_TOL under DRAWS re-solves with every
           input multiplied by 1 + PERTURB * U(-1, 1) (default_rng(7); LIP: x0, ref, foot; SRB-12: x0, xref).  An agent
           whose own iteration count moves under a 1e-12 change of its inputs cannot be held to equal counts on another
           arithmetic; the others can, shifted or not.
  loose    the rest.

Counts of each case (oracle, CPU): agents, shifted, shifted and strict, shifted-strict-OPTIMAL, strict in all, NLP
statuses of the batch, most failed factorisations of one iteration, largest delta, exit rules of the shifted agents.
The table is printed by `PYTHONPATH=.:srb-cbf-nmpc_amd python tests/shift_cases.py`.

  case     agents shifted sh&strict sh&strict&OPT strict  NLP statuses       tries  max delta  exits of the shifted agents
  LIP
  n2         32      1       1         1          32    32x0                 5    2.6e1    converged 1
  n3         32      3       3         3          32    32x0                 8    2.0e3    converged 1, provisional 2
  n11        32     18      12        12          26    32x0                 9    5.9e4    converged 9, provisional 9
  c4         32     15      14        14          31    31x0 1x2             8    2.0e4    converged 7, provisional 7, maxit 1
  default    64     32      23        22          55    61x0 1x2 2x4         9    3.2e7    converged 17, provisional 12, near_shifted 1, maxit 2
  w4          8      3       2         2           7    7x0 1x2              8    1.4e4    provisional 2, maxit 1
  n20        16     12       8         8          12    14x0 2x2             8    3.8e22   converged 7, provisional 3, maxit 2
  sw1e5      32     13      11        11          30    32x0                 8    7.7e3    converged 5, provisional 7, maxit 1
  near       32     15      14        13          31    30x0 1x2 1x4         9    7.2e5    converged 8, provisional 5, near_shifted 1, maxit 1
  SRB-12
  n10        32      3       3         3          32    31x0 1x4             6    2.2e1    converged 3
  n20         8      2       2         2           8    8x0                  5    3.8e0    converged 2
No case shifts at the default Sw.  (n20, seed 5, at Sw = 3e5 keeps 5 of 11 shifted agents stable and fails the half rule:
the case runs at Sw = 1e5.  The 1e22 shift belongs to MAXIT agents whose barrier weights diverged first; at the 1e-13
probe n11 had 14 of 18 and sw1e5 12 of 13 shifted agents strict, `near` 13 of 15.  The SRB-12 N = 20 batch of 16 agents
has 9 shifted agents, 7 of them strict, but two MAXIT agents make its five oracle solves take half a minute: the case
is the 8-agent batch, whose solves end within 19 iterations.)
The weights cases (LIP_WEIGHTS on `default`, SRB12_WEIGHTS on SRB-12 n10): no agent shifted, every agent stable.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle
from srbnmpc import workload

# The probe.  First probed at 1e-13 (three draws).  On the GPU two strict shifted agents then ended at the oracle's point
# (2.5e-8) with other iteration counts: n11 agent 7 (48 against 35) and sw1e5 agent 2 (37 against 36).  Their traces
# (the kernel's nlpdbg record against ORC_NLP_TRACE) agree to four digits in every column, every delta included, until
# an unshifted iteration whose reduced matrix is positive definite by a pivot within round-off of zero -- steps of
# ap ~ 1e-4 (n11, iteration 15, where the step lengths part by 0.5 %) and ap ~ 1e-7 (sw1e5, iterations 10-11) -- and
# drift apart from there; the first factorisation decision to differ (n11, iteration 26, one try fewer) comes after.
# The oracle itself moves both agents' counts at 1e-13 with more draws (8 / 16) and at 1e-12 with three, so the probe
# is 1e-12: the size of the backward error that separates two factorisations of a ~100-variable system (n eps times a
# growth of some tens), which is what the condensed Gauss-Jordan and the full-space LU are to each other.
PERTURB = 1e-12
DRAWS = 3
STABLE_TOL = 1e-7
SW_DEFAULT = 3000.0          # orc_params.Sw / orc12_params.Sw (MPC_dist.cpp:168-178)

LIP = {
    # name: N, C, K_obs, K_nbr, agents, waves asked for (0 automatic), waves expected, seed, Sw
    # the shapes of tests/test_gpu_factor_chain.py SHAPES (which variant of the factor and solve code each one is, there),
    # on crowded(A, N, C, seed) with Sw raised; n2 / n3 have one and three shifted agents (exempt from the half rule)
    "n2": (2, 2, 3, 8, 32, 1, 1, 5, 3e5),
    "n3": (3, 2, 3, 8, 32, 1, 1, 5, 3e5),
    "n11": (11, 2, 3, 8, 32, 1, 1, 5, 3e5),
    "c4": (5, 4, 3, 8, 32, 1, 1, 5, 3e5),
    "default": (10, 2, 3, 8, 64, 1, 1, 5, 3e5),
    "w4": (10, 2, 3, 0, 8, 0, 4, 5, 3e5),
    "n20": (20, 2, 3, 8, 16, 2, 2, 5, 1e5),
    "sw1e5": (10, 2, 3, 8, 32, 1, 1, 5, 1e5),
    # the `near && delta != 0` exit: agent 17 shifts at a near-optimal iterate and ends ACCEPTABLE, and is strict
    "near": (10, 2, 3, 8, 32, 1, 1, 12, 1e5),
}

# cases whose purpose is an exit rule of the shift loop (the scan of tools/shift_scan.py: 64 seeds x Sw in {3e4, 1e5, 3e5,
# 1e6} at N = 10, 32 agents); name -> the oracle.EXIT_RULES entry a strict shifted agent of the case leaves through and
# the NLP status it ends with.  The scan found 11 near_shifted agents (seeds 3, 8, 9, 12, 18, 21, 28, 45, 46, 59, 62) and
# none that exhausts the 14 tries (KKTFAIL): that exit has no case.
LIP_EXITS = {"near": ("near_shifted", 4)}

SRB12 = {
    # name: N, K_obs, K_nbr, agents, seed, Sw   (make_batch12 "trot", the crowded obstacle count)
    "n10": (10, 3, 8, 32, 5, 3e5),
    "n20": (20, 3, 8, 8, 5, 3e5),
}

# non-default weights that leave the batch unshifted (asserted on the CPU): every cost weight and eps_obs off its default
LIP_WEIGHTS = dict(Qw=450.0, Pw=1400.0, Rw=0.25, Sw=4500.0, eps_obs=1.6)
SRB12_WEIGHTS = dict(q_scale=1.5, qN_scale=0.75, r_scale=2.0, Sw=4500.0)

_cache = {}


def n_crowded(A):
    return int(round(80 * workload.arena_scale(A) ** 2))


def lip_batch(name):
    if ("lb", name) not in _cache:
        N, C, Ko, Kn, A, _, _, seed, _ = LIP[name]
        _cache[("lb", name)] = workload.make_batch(A, N, C, seed=seed, n_obs=n_crowded(A))
    return _cache[("lb", name)]


def lip_params(name, **kw):
    N, C, Ko, Kn = LIP[name][:4]
    kw.setdefault("Sw", LIP[name][8])
    return oracle.params(N, C, K_obs=Ko, K_nbr=Kn, use_nlp=1, **kw)


def _lip_solve(p, b, stats=False):
    return oracle.solve_batch(p, b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], nthreads=8, stats=stats)


def srb12_batch(name):
    if ("sb", name) not in _cache:
        N, Ko, Kn, A, seed, _ = SRB12[name]
        _cache[("sb", name)] = workload.make_batch12(A, N, "trot", seed=seed, n_obs=n_crowded(A))
    return _cache[("sb", name)]


def srb12_weights(p, q_scale=1.0, qN_scale=1.0, r_scale=1.0, Sw=None):
    """Scale the q, qN, r arrays of a Params12 / Orc12Params in place (both structures have the same fields)."""
    for i in range(12):
        p.q[i] *= q_scale
        p.qN[i] *= qN_scale
    for i in range(3):
        p.r[i] *= r_scale
    if Sw is not None:
        p.Sw = Sw
    return p


def srb12_params(name, **kw):
    N, Ko, Kn = SRB12[name][:3]
    kw.setdefault("Sw", SRB12[name][5])
    return srb12_weights(oracle.params12(N, K_obs=Ko, K_nbr=Kn), **kw)


def _srb12_solve(p, b, stats=False):
    return oracle.solve_batch12(p, b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"], b["nbr_state"], nthreads=8,
                                stats=stats)


def _xus(nx, x):
    """States, inputs and slack of a solution vector (LIP: lambda left out, not unique for C = 4): nx leading entries."""
    return np.concatenate([x[..., :nx], x[..., -1:]], -1)


def perturbed(b, keys):
    """DRAWS copies of batch b with the arrays `keys` multiplied by 1 + PERTURB * U(-1, 1) (default_rng(7), in order)."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(DRAWS):
        bp = dict(b)
        for k in keys:
            bp[k] = b[k] * (1.0 + PERTURB * rng.uniform(-1.0, 1.0, np.shape(b[k])))
        out.append(bp)
    return out


def solve_all(jobs):
    """The oracle solves `jobs` (callables) side by side: the library releases the interpreter and keeps no state."""
    with ThreadPoolExecutor(len(jobs)) as ex:
        return [f.result() for f in [ex.submit(j) for j in jobs]]


def stable_agents(r, draws, nx):
    """Agents of the oracle result r whose status, iteration counts and X, U, s survive the perturbed re-solves."""
    ok = np.ones(r["status"].shape[0], bool)
    for q in draws:
        ok &= (q["status"] == r["status"]).all(1) & (q["iters"] == r["iters"]).all(1)
        ok &= np.abs(_xus(nx, q["x"]) - _xus(nx, r["x"])).max(1) <= STABLE_TOL
    return ok


def _case(solve, b, keys, p, p0, nx):
    """r (params p, with stats), r0 (params p0, the default Sw; None: left out) and the stable agents of r."""
    jobs = [lambda: solve(p, b, stats=True)] + [lambda bp=bp: solve(p, bp) for bp in perturbed(b, keys)]
    if p0 is not None:
        jobs.append(lambda: solve(p0, b, stats=True))
    res = solve_all(jobs)
    r, draws, r0 = res[0], res[1:1 + DRAWS], res[-1] if p0 is not None else None
    strict = stable_agents(r, draws, nx)
    if r0 is None:
        return dict(r=r, strict=strict)
    return dict(r=r, r0=r0, shifted=r["stats"]["failed"] > 0, strict=strict, loose=~strict,
                shifted0=r0["stats"]["failed"] > 0)


def lip_case(name):
    """The oracle's solve of the case (r, with stats), of the same batch at the default Sw (r0), and the three sets as
    boolean arrays over the agents; computed once per session and shared -- read only."""
    if ("lc", name) not in _cache:
        _cache[("lc", name)] = _case(_lip_solve, lip_batch(name), ("x0", "ref", "foot"), lip_params(name),
                                     lip_params(name, Sw=SW_DEFAULT), 6 * LIP[name][0])
    return _cache[("lc", name)]


def srb12_case(name):
    if ("sc", name) not in _cache:
        _cache[("sc", name)] = _case(_srb12_solve, srb12_batch(name), ("x0", "xref"), srb12_params(name),
                                     srb12_params(name, Sw=SW_DEFAULT), 24 * SRB12[name][0])
    return _cache[("sc", name)]


def lip_weights_case():
    """The `default` shape with LIP_WEIGHTS: the oracle result (with stats) and the stable agents."""
    if "lw" not in _cache:
        _cache["lw"] = _case(_lip_solve, lip_batch("default"), ("x0", "ref", "foot"), lip_params("default", **LIP_WEIGHTS),
                             None, 60)
    return _cache["lw"]


def srb12_weights_case():
    if "sw" not in _cache:
        _cache["sw"] = _case(_srb12_solve, srb12_batch("n10"), ("x0", "xref"), srb12_params("n10", **SRB12_WEIGHTS), None, 240)
    return _cache["sw"]


def counts(c):
    """One line of the table above."""
    r, sh, st = c["r"], c["shifted"], c["strict"]
    s1 = r["status"][:, 1]
    ex = r["stats"]["exit"][sh]
    return dict(agents=int(sh.size), shifted=int(sh.sum()), shifted_strict=int((sh & st).sum()),
                shifted_strict_optimal=int((sh & st & (s1 == 0)).sum()), strict=int(st.sum()),
                statuses={int(k): int(v) for k, v in zip(*np.unique(s1, return_counts=True))},
                max_tries=int(r["stats"]["max_tries"].max()), max_delta=float(r["stats"]["max_delta"].max()),
                exits={oracle.EXIT_RULES[int(k)]: int(v) for k, v in zip(*np.unique(ex, return_counts=True))},
                shifted_at_default=int(c["shifted0"].sum()))


if __name__ == "__main__":
    for nm in LIP:
        print("LIP  ", nm, counts(lip_case(nm)), flush=True)
    for nm in SRB12:
        print("SRB12", nm, counts(srb12_case(nm)), flush=True)
    for nm, c in (("LIP weights", lip_weights_case()), ("SRB12 weights", srb12_weights_case())):
        print(nm, "shifted", int((c["r"]["stats"]["failed"] > 0).sum()), "strict", int(c["strict"].sum()), "of", c["strict"].size,
              "statuses", np.unique(c["r"]["status"][:, 1], return_counts=True))
