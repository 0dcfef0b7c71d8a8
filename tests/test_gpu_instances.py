"""GPU matrix over every shipped LIP-mode kernel instance (SRB_KERNEL_INSTANCES, csrc/srb_kernel_params.h): each
instance's solve kernel, polish kernel, table ("mv") solve kernel and table polish kernel, and the two fp32-factor
instances in both forms, each launched by a test of its own and held to the oracle.  What a case launched is not
argued: BatchSolver.last_kernels() reports the kernels' names from the launch site, and every case asserts them before
it compares anything.  The last test holds the union of the names seen against srbnmpc.kernel_table().

Cases (tests/instance_cases.py): per instance its smallest shape and its edges, waves forced with set_waves, 8 agents
(K_nbr = 0 throughout: K <= 16).  Forms:
  kernel   polish_fused = 0, polish_waves = the instance's NW: the instance's solve kernel and its own polish kernel,
           against oracle.solve_batch
  fused    the default fused polish (NZL <= 24): the fused arm of the same solve kernel, against oracle.solve_batch
  tabled   a non-zero velocity table (workload.obstacle_velocities, 1 m/s), polish_fused = 0: the mv solve and mv polish
           kernels, against moving_oracle.solve.  A shape with K = 0 has no column that reads a table (the host then
           launches the plain kernels), so its tabled form runs at K_obs = 1, which lands on the same instance.
  f32      kkt_fp32_mu = 0.1 on the two instances that have an fp32-factor variant, plain and tabled

Comparison rule (tests/test_gpu_parity.py test_gpu_matches_oracle, tests/test_gpu_gram_valu.py check_parity): statuses
equal; iteration counts equal on >= 85 % of the agents and nowhere more than 2 apart; X, U, s within 1e-4, within 1e-6
where both sides end NLP OPTIMAL; obj within rtol 1e-7 / atol 1e-6; sel equal.  On the oracle alone at least half of
a case's agents end NLP OPTIMAL and none KKTFAIL (asserted).
"""
import numpy as np
import pytest

import instance_cases as ic

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402

NLP_TOL = 1e-4
POLISHED_TOL = 1e-6

CASES = ic.lip_cases()
_seen = set()          # every kernel name a case saw through last_kernels()
_ran = set()           # the cases that were started (the last test needs all of them)


def name_of(prefix, dims):
    return prefix + "_".join(map(str, dims))


def case_id(dims, shape):
    return "%d_%d_%d-N%dC%dK%d" % (dims[:3] + tuple(shape))


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


def gpu_solve(dims, shape, want, options, vel=None):
    """One launch of `shape` at the instance's waves; `want` = (solve, polish) kernel names, asserted first."""
    N, C, K = shape
    Ko, Kn = ic.split_K(K)
    b = ic.lip_batch(shape)
    A = b["x0"].shape[0]
    assert A == ic.agents(K) >= Kn + 1 and b["obstacles"].shape[0] >= Ko            # neither K is clamped
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        s.set_waves(dims[2])
        for k, v in options.items():
            s.set_option(k, v)
        kw = {} if vel is None else dict(obs_vel=vel)
        out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], **kw)
        out = {k: np.array(v, copy=True) for k, v in out.items() if v is not None}
        got = s.last_kernels()
        _seen.update(n for n in got if n)
        assert got == want, (got, want)
        assert s.waves() == dims[2]
        assert s.get_option("last_polish") == (1.0 if want[1] else 2.0)
        out["last_kkt_fp32"] = s.get_option("last_kkt_fp32")
    finally:
        s.close()
    return out


def check(N, out, r):
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    same = np.all(out["iters"] == r["iters"], 1)
    print("max |X,U,s - oracle| per agent:", e.max(), "statuses", np.unique(out["status"], axis=0, return_counts=True),
          "iterations equal on", same.mean(), "largest count difference", int(np.abs(out["iters"] - r["iters"]).max()),
          "max |obj - oracle|", np.abs(out["obj"] - r["obj"]).max())
    assert ic.oracle_is_fit(r), np.unique(r["status"], axis=0, return_counts=True)
    np.testing.assert_array_equal(out["status"], r["status"])
    assert same.mean() >= 0.85, same
    assert np.abs(out["iters"] - r["iters"]).max() <= 2
    assert e.max() < NLP_TOL, (int(np.argmax(e)), float(e.max()))
    both = (out["status"][:, 1] == 0) & (r["status"][:, 1] == 0)
    assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))
    np.testing.assert_allclose(out["obj"], r["obj"], rtol=1e-7, atol=1e-6)
    assert np.array_equal(out["sel"], r["sel"])


def table_matters(N, shape):
    """The moving answer differs from the static one of the same batch by more than 1e-3 on at least one agent of the
    eight (tests/test_gpu_stage_bodies.py test_moving_obstacle_form: four of 32)."""
    r, r0 = ic.lip_moving(shape), ic.lip_plain(shape)
    assert (np.abs(r["x"][:, :6 * N] - r0["x"][:, :6 * N]).max(1) > 1e-3).sum() >= 1


@pytest.mark.parametrize("dims,shape", CASES, ids=[case_id(d, s) for d, s in CASES])
def test_solve_and_polish_kernel(dims, shape):
    _ran.add(("kernel", dims, shape))
    want = (name_of("srb_nmpc_kernel_", dims), name_of("srb_polish_kernel_", dims))
    out = gpu_solve(dims, shape, want, {"polish_fused": 0, "polish_waves": dims[2]})
    check(shape[0], out, ic.lip_plain(shape))


FUSED = [(d, s) for d, s in CASES if d[0] <= 24]


@pytest.mark.parametrize("dims,shape", FUSED, ids=[case_id(d, s) for d, s in FUSED])
def test_fused_polish(dims, shape):
    _ran.add(("fused", dims, shape))
    out = gpu_solve(dims, shape, (name_of("srb_nmpc_kernel_", dims), ""), {})
    check(shape[0], out, ic.lip_plain(shape))


@pytest.mark.parametrize("dims,shape", CASES, ids=[case_id(d, s) for d, s in CASES])
def test_table_kernels(dims, shape):
    _ran.add(("tabled", dims, shape))
    shape = ic.tabled_shape(shape)
    if dims[3]:
        assert shape == dims[3:]
    want = (name_of("srb_nmpc_kernel_mv_", dims), name_of("srb_polish_kernel_mv_", dims))
    table_matters(shape[0], shape)
    out = gpu_solve(dims, shape, want, {"polish_fused": 0, "polish_waves": dims[2]}, vel=ic.lip_velocities(shape))
    check(shape[0], out, ic.lip_moving(shape))


@pytest.mark.parametrize("tabled", [False, True], ids=["plain", "tabled"])
@pytest.mark.parametrize("dims", ic.LIP_F32, ids=[name_of("", d) for d in ic.LIP_F32])
def test_fp32_factor_instances(dims, tabled):
    """kkt_fp32_mu = 0.1: srb_nmpc_kernel_f32_* / srb_nmpc_kernel_mv_f32_* (the reduced matrix inverted in fp32 while
    mu > 0.1, every solve refined in fp64), polished by the fused arm; the same rule against the same references."""
    _ran.add(("f32", dims, tabled))
    shape = dims[3:]
    want = (name_of("srb_nmpc_kernel_mv_f32_" if tabled else "srb_nmpc_kernel_f32_", dims), "")
    out = gpu_solve(dims, shape, want, {"kkt_fp32_mu": 0.1}, vel=ic.lip_velocities(shape) if tabled else None)
    assert out["last_kkt_fp32"] == 1.0
    check(shape[0], out, ic.lip_moving(shape) if tabled else ic.lip_plain(shape))


def test_every_shipped_kernel_was_launched():
    """The names seen through last_kernels() over this file are the shipped LIP solve kernels: kernel_table() and the
    polish, mv and mv-polish names of its fp64 entries, the mv names of its f32 entries."""
    n_cases = 2 * len(CASES) + len(FUSED) + 2 * len(ic.LIP_F32)
    if len(_ran) != n_cases:
        pytest.skip(f"{n_cases - len(_ran)} of {n_cases} cases were deselected")
    want = set()
    for dims, name in srbnmpc.kernel_table():
        assert name == name_of("srb_nmpc_kernel_f32_" if "_f32_" in name else "srb_nmpc_kernel_", dims)
        if "_f32_" in name:
            want |= {name, name_of("srb_nmpc_kernel_mv_f32_", dims)}
        else:
            want |= {name, name_of("srb_polish_kernel_", dims), name_of("srb_nmpc_kernel_mv_", dims),
                     name_of("srb_polish_kernel_mv_", dims)}
    assert _seen == want, (sorted(want - _seen), sorted(_seen - want))
