"""CPU tests of obstacle sizes in the SRB-12 mode (srb_sizes through srb12_solve_batch_sized[_device],
srb12_sim_metrics_sized_device, srb12_rollout_sized_device): the two-level reference of tests/sizes12_oracle.py against
the oracle's own answers, the check that it and the per-column certificate discriminate, the names, and the refusals
and the Python layer's validation that need no context (tests/test_sizes12_gpu.py then holds the device against the
references; the ValueErrors of Rollout12, which needs device tensors, are there)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import moving12_oracle as mo
import oracle
import plan12_oracle as po
import sizes12_oracle as so
import srbnmpc
from srbnmpc import srb12

NEW_NAMES = ("srb12_solve_batch_sized", "srb12_solve_batch_sized_device", "srb12_sim_metrics_sized_device",
             "srb12_rollout_sized_device")
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
# measured with the oracle alone: agents whose selected rows carry both levels, and agents whose X moves by more than
# 1e-4 against the unsized answer
MIXED = {mo.SHAPES0[0]: 11, mo.SHAPES0[1]: 0, mo.SHAPES0[2]: 5, mo.SHAPES0[3]: 4}
MOVED = {mo.SHAPES0[0]: 9, mo.SHAPES0[1]: 5, mo.SHAPES0[2]: 7, mo.SHAPES0[3]: 5}


# ================================================================================== the two-level reference
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_two_level_reference_on_a_uniform_table_is_the_oracle_both_ways_round(shape):
    """Every row at eps_obs: handed over as the static table (e0 = eps_obs) or as the zero-velocity neighbour table
    (e1 = eps_obs), the helper returns oracle.solve_batch12's x, obj and status."""
    R = so.reference(shape)
    b, p, r0 = R["b"], R["p"], R["r0"]
    uni = np.full(b["obstacles"].shape[0], p.eps_obs)
    for levels in ((p.eps_obs, 0.25), (0.25, p.eps_obs)):
        r = so.solve_two_level(p, b, b["obstacles"], uni, R["sel"], levels)
        assert np.array_equal(r["status"], r0["status"]), levels
        assert np.array_equal(r["x"], r0["x"]) and np.array_equal(r["obj"], r0["obj"]), levels


@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_two_level_reference_and_the_certificate_discriminate(shape):
    """On the two-level table every solve converges, the answer moves, the certificate with the gathered levels is
    inside the thresholds for every agent, and with uniform levels it is beyond them on at least one."""
    N, Ko, A, gait, seed = shape
    R = so.reference(shape)
    b, p, r, eps, sel = R["b"], R["p"], R["r"], R["eps"], R["sel"]
    assert (r["status"] == np.array([4, 0])).all(), r["status"].tolist()
    lv = eps[sel]
    mixed = int((lv.min(1) != lv.max(1)).sum())
    moved = int((np.abs(r["x"][:, :12 * N] - R["r0"]["x"][:, :12 * N]).max(1) > 1e-4).sum())
    worst, wrong = dict(eq=0.0, prim=0.0, stat_rel=0.0), 0
    for a in range(A):
        obs, ep = so.rows_sized(p, b, a, None, sel[a], eps)
        assert np.array_equal(ep, eps[sel[a]])
        cert = po.certificate(p, b, a, obs, ep, r["x"][a])
        assert cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL, (a, cert)
        worst = {k: max(v, cert[k]) for k, v in worst.items()}
        bad = po.certificate(p, b, a, obs, np.full(Ko, p.eps_obs), r["x"][a])
        wrong += not (bad["eq"] < EQ_TOL and bad["prim"] < PRIM_TOL and bad["stat_rel"] < STAT_TOL)
    print(f"shape {shape}: {mixed} agents with both levels, {moved} moved by more than 1e-4, worst certificate {worst}, "
          f"{wrong} of {A} beyond the thresholds with uniform levels")
    assert mixed == MIXED[shape] and moved == MOVED[shape]
    assert wrong >= 1


# ================================================================================== names
def test_header_declares_and_library_exports_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    L = srb12._lib()
    for n in NEW_NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(L, n), n
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert L.srb_abi_version() == 6 == srbnmpc.ABI_VERSION
    assert "The SRB-12 mode and the MPC_dist shims have no obstacle sizes" not in hdr
    for fn in (srb12.Solver12.solve, srb12.Solver12.solve_device, srb12.Solver12.solve_coupled_device):
        assert {"obs_eps", "obs_clearance"} <= set(inspect.signature(fn).parameters), fn
    assert {"obs_eps", "obs_radius", "obs_clearance"} <= set(inspect.signature(srb12.Rollout12.__init__).parameters)


# ================================================================================== refusals without a context
def test_refusals_that_need_no_gpu():
    """The refusals of srb_sizes are made by name (SRB_ERR_ARG = -1) with a NULL context, through each new entry
    point: nothing is launched."""
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    d = np.zeros(64)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    S, B = srbnmpc.Sizes, srb12.Batch12
    sim = srb12.Sim12(); sim.goal = ptr(d)
    calls = (lambda sz: lib.srb12_solve_batch_sized(None, 1, ctypes.byref(B()), None, None, ctypes.byref(sz)),
             lambda sz: lib.srb12_solve_batch_sized_device(None, 1, ctypes.byref(B()), None, None, ctypes.byref(sz), None),
             lambda sz: lib.srb12_sim_metrics_sized_device(None, 1, ctypes.byref(sim), ctypes.byref(sz), 0, None),
             lambda sz: lib.srb12_rollout_sized_device(None, 1, ctypes.byref(B()), ctypes.byref(sim), None, None,
                                                       ctypes.byref(sz), 1, None))
    for fn in calls:
        for bad in (0, ctypes.sizeof(S) - 8, ctypes.sizeof(S) + 8, ctypes.sizeof(B)):
            sz = S(); sz.struct_size = bad
            assert fn(sz) == -1 and "srb_sizes.struct_size" in err()
        for bad in (2, -1):
            assert fn(S(ptr(d), None, bad)) == -1 and "srb_sizes.clearance_selection: 0" in err()
        assert fn(S(None, ptr(d), 1)) == -1 and "clearance_selection = 1 needs obs_eps" in err()
        assert fn(S(ptr(d), ptr(d), 1)) == -1 and "null argument" in err()      # a good srb_sizes: the entry extended
        assert fn(S()) == -1 and "null argument" in err()
    # what the extended entry points refuse comes through as well
    mv = srbnmpc.Moving(None, 1, None)
    assert lib.srb12_solve_batch_sized_device(None, 1, ctypes.byref(B()), None, ctypes.byref(mv), ctypes.byref(S()),
                                              None) == -1 and "horizon_selection = 1 needs obs_vel" in err()
    b = B(); b.struct_size += 8
    assert lib.srb12_rollout_sized_device(None, 1, ctypes.byref(b), ctypes.byref(sim), None, None, ctypes.byref(S()), 1,
                                          None) == -1 and "srb12_batch.struct_size" in err()


def test_python_layer_validates_by_name_without_a_context():
    """obs_eps is checked before the library (or the context) is touched: a Solver12 that was never created serves.
    obs_clearance without obs_eps is the library's refusal, made by name before it touches the (null) context."""
    s = srb12.Solver12.__new__(srb12.Solver12)
    s.params, s._scenes, s._h = srb12.default_params(10, K_obs=1, K_nbr=0), (0, 0), None
    s.max_agents, s.device = 8, 0
    A, N, n_obs = 4, 10, 5
    x0, xref, foot = np.zeros((A, 12)), np.zeros((A, N, 12)), np.zeros((A, N, 4, 3))
    contact, ob = np.zeros((A, N, 4), np.int32), np.zeros((n_obs, 2))
    for bad in (np.zeros(n_obs, np.float32), np.zeros((n_obs, 1)), np.zeros(n_obs + 1), np.zeros(2 * n_obs)[::2],
                [1.0] * n_obs):
        with pytest.raises(ValueError, match="obs_eps must be a contiguous float64 array"):
            s.solve(x0, xref, foot, contact, ob, obs_eps=bad)
    with pytest.raises(ValueError, match="obs_eps must be a contiguous float64 array"):
        s.solve(x0, xref, foot, contact, None, obs_eps=np.ones(n_obs))            # a table without obstacles
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs obs_eps") as e:
        s.solve(x0, xref, foot, contact, ob, obs_clearance=True)
    assert "srbnmpc error -1:" in str(e.value)
    q = srb12.Solver12.__new__(srb12.Solver12)
    q.params, q._scenes, q._h = srb12.default_params(10, K_obs=1, K_nbr=0, use_nlp=0), (0, 0), None
    with pytest.raises(ValueError, match="QP-only solve has no obstacle rows"):
        q.solve(x0, xref, foot, contact, ob, obs_eps=np.ones(n_obs))
    torch = pytest.importorskip("torch")
    t = lambda a: torch.as_tensor(a)
    out = dict(x=t(np.zeros((A, 241))), obj=t(np.zeros(A)), status=t(np.zeros((A, 2), np.int32)),
               iters=t(np.zeros((A, 2), np.int32)))
    args = (t(x0), t(xref), t(foot), t(contact), t(ob), None)
    for bad in (torch.zeros(n_obs, dtype=torch.float32), torch.zeros(n_obs + 1, dtype=torch.float64),
                torch.zeros(2 * n_obs, dtype=torch.float64)[::2], torch.zeros(n_obs, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="obs_eps must be"):
            s.solve_device(*args, out, obs_eps=bad)
        with pytest.raises(ValueError, match="obs_eps must be"):
            s.solve_coupled_device(*args, dict(out, plan=torch.zeros(A, N, 2, dtype=torch.float64)), outer=1, obs_eps=bad)
    with pytest.raises(ValueError, match="obs_eps must be"):
        s.solve_device(t(x0), t(xref), t(foot), t(contact), None, None, out, obs_eps=torch.ones(n_obs, dtype=torch.float64))
