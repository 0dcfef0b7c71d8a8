"""GPU matrix over every shipped SRB-12 kernel instance (SRB12_INSTANCES, csrc/srb_kernel_params.h): the solve kernel
and the table ("mv") kernel of each, launched by a test of its own at the shapes where the leg trips (4 N legs over 64
lanes) and the obstacle trips (N K rows) are exactly full, one over, and at their largest.  Every case asserts
Solver12.last_kernel(), the name recorded at the launch site, before it compares anything; the last test holds the
union of the names seen against srb12.kernel_table().

Cases (tests/instance_cases.py SHAPES12): K_obs = min(K, 16), K_nbr = K - K_obs, A = max(8, K_nbr + 1) trot agents of
workload.make_batch12, so that neither K is clamped.  No shape is refused by the 160 KiB LDS bound of
srb12_check_params (the largest, N = 24 with K = 32, carves 96 KiB), so none is reduced.

Plain cases: oracle.solve_batch12 by the rule of tests/test_srb12.py test_srb12_variants_vs_oracle (statuses equal,
states within 1e-6, forces within 1e-4 N).  Tabled cases (a velocity table of 1 m/s, workload.obstacle_velocities), at
the bounds of tests/test_moving12_gpu.py: with K_nbr = 0 moving12_oracle.solve_moving, the oracle's own answer
(statuses equal; X 1e-6, forces 1e-4 N, s 1e-6); with K_nbr > 0, which no oracle answers, every agent converges and its
point passes the KKT certificate of the rows built in numpy (eq < 1e-9, prim < 1e-7, stat_rel < 1e-6).  N = 6, K = 0
reads no table and has no tabled form.
"""
import numpy as np
import pytest

import instance_cases as ic
import moving12_oracle as mo
import plan12_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from srbnmpc import srb12  # noqa: E402

X_TOL, F_TOL, S_TOL = 1e-6, 1e-4, 1e-6                      # tests/test_srb12.py, tests/test_moving12_gpu.py
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate

# the instance each shape is meant for: (TL, TO, NC, K1)
WANT = {(16, 4): (1, 1, 0, 0), (17, 3): (2, 4, 0, 0), (8, 8): (1, 1, 0, 0), (16, 8): (1, 2, 0, 0), (16, 16): (1, 4, 0, 0),
        (16, 32): (1, 8, 0, 0), (20, 20): (2, 8, 0, 0), (24, 32): (2, 12, 0, 0), (10, 11): (1, 2, 10, 12),
        (20, 11): (2, 4, 20, 12), (6, 0): (1, 1, 0, 0)}
TABLED = [sh for sh in ic.SHAPES12 if sh[1] > 0]
_seen, _ran = set(), set()


def opt(st):
    return np.isin(st[:, 0], (0, 4)) & (st[:, 1] == 0)


def gpu_solve(shape, want, vel=None):
    N, K = shape
    Ko, Kn = ic.split_K(K)
    b = ic.batch12(shape)
    A = b["x0"].shape[0]
    assert A == ic.agents(K) >= Kn + 1 and b["obstacles"].shape[0] >= Ko            # neither K is clamped
    p = srb12.default_params(N, K_obs=Ko, K_nbr=Kn)
    assert srb12.check_params(p) and srb12.lds_bytes(p) <= 160 * 1024
    s = srb12.Solver12(p, A)
    try:
        kw = {} if vel is None else dict(obs_vel=vel)
        out = s.solve(b["x0"], b["xref"], b["foot"], b["contact"], b["obstacles"] if Ko else None,
                      b["nbr_state"] if Kn else None, **kw)
        out = {k: np.array(v, copy=True) for k, v in out.items() if v is not None}
        got = s.last_kernel()
        _seen.add(got)
        assert got == want, (got, want)
        assert out["sel"].shape == (A, K)
    finally:
        s.close()
    return out


def errors(N, got, want):
    return (np.abs(got[:, :12 * N] - want[:, :12 * N]).max(), np.abs(got[:, 12 * N:24 * N] - want[:, 12 * N:24 * N]).max(),
            np.abs(got[:, -1] - want[:, -1]).max())


@pytest.mark.parametrize("shape", ic.SHAPES12, ids=["N%dK%d" % sh for sh in ic.SHAPES12])
def test_solve_kernel(shape):
    _ran.add(("plain", shape))
    N, K = shape
    out = gpu_solve(shape, "srb12_kernel_" + "_".join(map(str, WANT[shape])))
    b, r = ic.batch12(shape), ic.plain12(shape)
    assert ic.oracle_is_fit(r), np.unique(r["status"], axis=0, return_counts=True)
    ex, eu, es = errors(N, out["x"], r["x"])
    print(f"shape {shape}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; statuses", np.unique(out["status"], axis=0, return_counts=True))
    np.testing.assert_array_equal(out["status"], r["status"])
    np.testing.assert_allclose(out["x"][:, :12 * N], r["x"][:, :12 * N], atol=X_TOL)
    np.testing.assert_allclose(out["x"][:, 12 * N:], r["x"][:, 12 * N:], atol=F_TOL)


@pytest.mark.parametrize("shape", TABLED, ids=["N%dK%d" % sh for sh in TABLED])
def test_table_kernel(shape):
    _ran.add(("tabled", shape))
    N, K = shape
    Ko, Kn = ic.split_K(K)
    b, w = ic.batch12(shape), ic.velocities12(shape)
    out = gpu_solve(shape, "srb12_kernel_mv_" + "_".join(map(str, WANT[shape])), vel=w)
    if Kn == 0:
        r, r0 = ic.moving12(shape), ic.plain12(shape)
        assert ic.oracle_is_fit(r), np.unique(r["status"], axis=0, return_counts=True)
        assert not np.array_equal(r["x"], r0["x"])                                  # the table matters
        ex, eu, es = errors(N, out["x"], r["x"])
        print(f"shape {shape}: max |X| {ex:.3e} |U| {eu:.3e} |s| {es:.3e}; statuses", np.unique(out["status"], axis=0, return_counts=True))
        assert np.array_equal(out["status"], r["status"]), (out["status"].tolist(), r["status"].tolist())
        assert ex < X_TOL and eu < F_TOL and es < S_TOL, (ex, eu, es)
        assert np.array_equal(out["sel"], mo.snapshot_select(b, b["obstacles"], Ko))
        return
    p = ic.params12(shape)
    ok = opt(out["status"])
    worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
    for a in np.where(ok)[0]:
        obs, eps = mo.rows_moving(p, b, a, None, out["sel"][a], b["obstacles"], w)
        cert = po.certificate(p, b, a, obs, eps, out["x"][a])
        assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
    print(f"shape {shape}: {ok.sum()}/{len(ok)} converged, worst certificate {worst}")
    assert ok.all(), (np.where(~ok)[0].tolist(), out["status"][~ok].tolist())
    assert not np.array_equal(out["x"], gpu_solve(shape, "srb12_kernel_" + "_".join(map(str, WANT[shape])))["x"])   # the table matters


def test_every_shipped_kernel_was_launched():
    n_cases = len(ic.SHAPES12) + len(TABLED)
    if len(_ran) != n_cases:
        pytest.skip(f"{n_cases - len(_ran)} of {n_cases} cases were deselected")
    want = set()
    for dims, name in srb12.kernel_table():
        want |= {name, "srb12_kernel_mv_" + "_".join(map(str, dims))}
    assert _seen == want, (sorted(want - _seen), sorted(_seen - want))
