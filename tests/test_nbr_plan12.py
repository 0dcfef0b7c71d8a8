"""CPU tests of the neighbour plans of the SRB-12 mode (srb12_plans): the new names, the layout of the ctypes
mirror, the refusals that need no context, the helpers of tests/plan12_oracle.py against the oracle's own pieces,
and the check that the linear-table reference discriminates (tests/test_nbr_plan12_gpu.py then holds the device
against these references)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import oracle
import plan12_oracle as po
import srbnmpc
from srbnmpc import dist as sdist
from srbnmpc import srb12
from test_srb12 import _opt

NEW_NAMES = ("srb12_solve_batch_plans", "srb12_solve_batch_plans_device", "srb12_shift_plans_device",
             "srb12_rollout_plans_device")
# agents whose X moves by more than 1e-4 between the two oracle runs, measured with the oracle alone (at least one
# is asserted, so that a later change of seeds cannot empty the GPU test)
MOVED = {po.SHAPES12[0]: 1, po.SHAPES12[1]: 5, po.SHAPES12[2]: 6, po.SHAPES12[3]: 2, po.SHAPES12[4]: 2}


# ================================================================================== names and layout
def test_header_declares_and_library_exports_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    L = srbnmpc.lib()
    for n in NEW_NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(L, n), n
    assert "typedef struct srb12_plans {" in hdr
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert L.srb_abi_version() == 6 == srbnmpc.ABI_VERSION


def test_plans12_layout_matches_the_header(tmp_path):
    names = [f for f, _ in srb12.Plans12._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(srb12_plans), sizeof(srb12_batch), sizeof(srb12_sim));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(srb12_plans, {n}));\n' for n in names) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = srb12.Plans12
    assert got[0] == ctypes.sizeof(P)
    assert got[1] == ctypes.sizeof(srb12.Batch12) and got[2] == ctypes.sizeof(srb12.Sim12)     # the old layouts stay
    assert got[3:] == [getattr(P, n).offset for n in names]
    assert names == ["struct_size", "nbr_plan", "plan", "plan_selection", "plan_table"]
    assert P().struct_size == ctypes.sizeof(P)


# ================================================================================== refusals without a context
def test_refusals_that_need_no_gpu():
    """Every refusal that needs no context is made by name (SRB_ERR_ARG = -1) with a NULL context, so nothing is
    launched and no context is looked at."""
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    d = np.zeros(64)
    e = np.zeros(64)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    solves = (lambda b, pl: lib.srb12_solve_batch_plans(None, 1, ctypes.byref(b), ctypes.byref(pl)),
              lambda b, pl: lib.srb12_solve_batch_plans_device(None, 1, ctypes.byref(b), ctypes.byref(pl), None))
    roll = lambda b, s, pl: lib.srb12_rollout_plans_device(None, 1, ctypes.byref(b), ctypes.byref(s), ctypes.byref(pl), 1, None)
    size = ctypes.sizeof(srb12.Plans12)
    for fn in solves:
        for bad in (0, size - 8, size + 8, ctypes.sizeof(srb12.Batch12)):
            pl = srb12.Plans12(); pl.struct_size = bad
            assert fn(srb12.Batch12(), pl) == -1 and "srb12_plans.struct_size" in err()
        b = srb12.Batch12(); b.struct_size += 8
        assert fn(b, srb12.Plans12()) == -1 and "srb12_batch.struct_size" in err()
        # nbr_plan without nbr_state
        pl = srb12.Plans12(); pl.nbr_plan = ptr(d)
        assert fn(srb12.Batch12(), pl) == -1 and "nbr_plan needs nbr_state" in err()
        # plan_selection = 1 without nbr_plan, and a value that is neither
        pl = srb12.Plans12(); pl.plan_selection = 1
        assert fn(srb12.Batch12(), pl) == -1 and "plan_selection = 1 needs nbr_plan" in err()
        pl.plan_selection = 2
        assert fn(srb12.Batch12(), pl) == -1 and "plan_selection: 0" in err()
        # plan == nbr_plan, plan == plan_table
        b = srb12.Batch12(); b.nbr_state = ptr(e); b.n_all = 1
        pl = srb12.Plans12(); pl.nbr_plan = ptr(d); pl.plan = ptr(d)
        assert fn(b, pl) == -1 and "plan overlaps the nbr_plan table" in err()
        pl = srb12.Plans12(); pl.plan = ptr(d); pl.plan_table = ptr(d)
        assert fn(b, pl) == -1 and "plan overlaps plan_table" in err()
        # all of them passed: the NULL context is the next thing looked at
        pl = srb12.Plans12(); pl.nbr_plan = ptr(d); pl.plan = ptr(e)
        assert fn(b, pl) == -1 and "null argument" in err()
    assert lib.srb12_solve_batch_plans(None, 1, ctypes.byref(srb12.Batch12()), None) == -1 and "null argument" in err()
    # the shift
    assert lib.srb12_shift_plans_device(None, 1, ptr(d), -1, ptr(e), None) == -1 and "grids must be >= 0" in err()
    assert lib.srb12_shift_plans_device(None, 1, None, 4, ptr(e), None) == -1 and "missing buffer" in err()
    assert lib.srb12_shift_plans_device(None, 1, ptr(d), 4, ptr(d), None) == -1 and "two buffers" in err()
    assert lib.srb12_shift_plans_device(None, 1, ptr(d), 4, ptr(e), None) == -1 and "null argument" in err()
    # the rollout driver
    sim = srb12.Sim12(); sim.goal = ptr(d)
    pl = srb12.Plans12(); pl.struct_size += 8
    assert roll(srb12.Batch12(), sim, pl) == -1 and "srb12_plans.struct_size" in err()
    s2 = srb12.Sim12(); s2.struct_size -= 8
    assert roll(srb12.Batch12(), s2, srb12.Plans12()) == -1 and "srb12_sim.struct_size" in err()
    assert roll(srb12.Batch12(), srb12.Sim12(), srb12.Plans12()) == -1 and "goal" in err()
    assert roll(srb12.Batch12(), sim, srb12.Plans12()) == -1 and "needs srb12_plans.plan and plan_table" in err()
    pl = srb12.Plans12(); pl.plan = ptr(d); pl.plan_table = ptr(d)
    assert roll(srb12.Batch12(), sim, pl) == -1 and "plan overlaps plan_table" in err()
    pl = srb12.Plans12(); pl.plan = ptr(d); pl.plan_table = ptr(e); pl.nbr_plan = ptr(d)
    assert roll(srb12.Batch12(), sim, pl) == -1 and "plan overlaps the nbr_plan table" in err()
    pl.nbr_plan = None
    assert roll(srb12.Batch12(), sim, pl) == -1 and "null argument" in err()


def test_python_layer_validates_plan_arrays_before_the_library():
    """Solver12.solve / solve_device / shift_plans_device and Rollout12 check shapes, dtypes and contiguity with
    _check_plan_array before the library (or the context) is touched: a Solver12 that was never created serves."""
    s = srb12.Solver12.__new__(srb12.Solver12)
    s.params, s._scenes, s._h = srb12.default_params(10, K_obs=1, K_nbr=2), (0, 0), None
    A, N = 4, 10
    x0, xref, foot = np.zeros((A, 12)), np.zeros((A, N, 12)), np.zeros((A, N, 4, 3))
    contact, nbr = np.zeros((A, N, 4), np.int32), np.zeros((A, 4))
    for bad in (np.zeros((A, N, 2), np.float32), np.zeros((A, N, 3)), np.zeros((A + 1, N, 2)),
                np.zeros((A, N, 4))[:, :, ::2]):
        with pytest.raises(ValueError, match="nbr_plan must be a contiguous float64 array"):
            s.solve(x0, xref, foot, contact, None, nbr, nbr_plan=bad)
    torch = pytest.importorskip("torch")
    t = lambda a: torch.as_tensor(a)
    out = dict(x=t(np.zeros((A, 241))), obj=t(np.zeros(A)), status=t(np.zeros((A, 2), np.int32)),
               iters=t(np.zeros((A, 2), np.int32)))
    args = (t(x0), t(xref), t(foot), t(contact), None, t(nbr))
    with pytest.raises(ValueError, match="nbr_plan must be"):
        s.solve_device(*args, out, nbr_plan=torch.zeros(A, N, 2, dtype=torch.float32))
    with pytest.raises(ValueError, match="plan must be"):
        s.solve_device(*args, dict(out, plan=torch.zeros(A, N + 1, 2, dtype=torch.float64)))
    with pytest.raises(ValueError, match="plan must be"):
        s.solve_device(*args, out, plan=torch.zeros(A, N, 4, dtype=torch.float64)[:, :, ::2])
    with pytest.raises(ValueError, match=r"out\['plan'\]"):
        s.solve_coupled_device(*args, out)
    with pytest.raises(ValueError, match=r"out\['plan'\] must be"):
        s.solve_coupled_device(*args, dict(out, plan=torch.zeros(A, N, 2, dtype=torch.float32)))
    with pytest.raises(ValueError, match="table must be"):
        s.shift_plans_device(torch.zeros(A, N, 2, dtype=torch.float64), torch.zeros(A, N, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="plan must be"):
        s.shift_plans_device(torch.zeros(A, N, dtype=torch.float64), torch.zeros(A, N, 2, dtype=torch.float64))


# ================================================================================== the helpers
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_helper_table_and_rows_equal_the_oracle_prediction(shape):
    """The linear table built in numpy equals the oracle's own prediction rows for the snapshot (p_i, w_i) bit for
    bit, through `rows`; the snapshot selection is the same for both snapshots (it reads positions only)."""
    R = po.reference(shape)
    p, b = R["p"], R["b"]
    lin = dict(b, nbr_state=R["nbr_lin"])
    op = po.lip_params(p)
    for a in range(shape[3]):
        sel = po.select(p, b, a)
        assert np.array_equal(sel, po.select(p, lin, a))
        want, weps = oracle.select_obstacles(op, po.lip_x0(b["x0"][a]), b["obstacles"], R["nbr_lin"], a)
        obs, eps = po.rows(p, b, a, R["table"])
        assert np.array_equal(obs, want) and np.array_equal(eps, weps), a
        want_cv, _ = oracle.select_obstacles(op, po.lip_x0(b["x0"][a]), b["obstacles"], b["nbr_state"], a)
        assert np.array_equal(po.rows(p, b, a, None)[0], want_cv), a
        assert np.array_equal(po.rows(p, b, a, po.cv_table(p, b["nbr_state"]))[0], want_cv), a


def test_helper_shift_equals_dist_shift_plans():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    for N in (2, 4, 5, 10):
        plan = rng.normal(size=(7, N, 2))
        for g in (0, 1, 4, N, N + 3):
            want = sdist.shift_plans(torch.as_tensor(plan), g).numpy()
            assert np.array_equal(po.shift(plan, g), want), (N, g)
    assert np.array_equal(po.shift(plan, 0), plan)
    x = rng.normal(size=(3, 24 * 4 + 1))
    assert np.array_equal(po.plans_of(4, x)[1, 2], x[1, [24, 25]])


# ================================================================================== the reference discriminates
@pytest.mark.parametrize("shape", po.SHAPES12)
def test_linear_table_reference_converges_and_discriminates(shape):
    """Every agent converges in both oracle runs, the two answers differ (a kernel that ignores the table fails the
    GPU test on every shape), and the oracle's point for the linear table passes the KKT certificate with rows built
    from the selection plus the table."""
    R = po.reference(shape)
    N, A = shape[0], shape[3]
    assert _opt(R["r_cv"]["status"]).all() and _opt(R["r_lin"]["status"]).all()
    d = np.abs(R["r_lin"]["x"][:, :12 * N] - R["r_cv"]["x"][:, :12 * N]).max(1)
    print(f"shape {shape}: {int((d > 1e-4).sum())} agents moved by more than 1e-4, max |dX| {d.max():.3f}")
    assert (d > 1e-4).sum() >= 1
    assert (d > 1e-4).sum() == MOVED[shape]
    a = int(np.argmax(d))
    obs, eps = po.rows(R["p"], R["b"], a, R["table"])
    cert = po.certificate(R["p"], R["b"], a, obs, eps, R["r_lin"]["x"][a])
    assert cert["eq"] < 1e-9 and cert["prim"] < 1e-7 and cert["stat_rel"] < 1e-6, cert


def test_constant_velocity_point_fails_the_certificate_of_the_linear_table():
    """The certificate sees the table: on the stand shape the constant-velocity solve's points are no KKT points of
    the problem with the linear table's rows for the agents that moved."""
    shape = po.SHAPES12[1]
    R = po.reference(shape)
    N = shape[0]
    d = np.abs(R["r_lin"]["x"][:, :12 * N] - R["r_cv"]["x"][:, :12 * N]).max(1)
    a = int(np.argmax(d))
    obs, eps = po.rows(R["p"], R["b"], a, R["table"])
    cert = po.certificate(R["p"], R["b"], a, obs, eps, R["r_cv"]["x"][a])
    assert not (cert["eq"] < 1e-9 and cert["prim"] < 1e-7 and cert["stat_rel"] < 1e-6), cert
