"""CPU tests of moving obstacles in the SRB-12 mode (srb_moving through srb12_solve_batch_moving[_device],
srb12_obstacles_advance_device, srb12_rollout_moving_device): the references of tests/moving12_oracle.py against the
oracle's own answers, the check that they discriminate, the names and layouts, and the refusals and the Python
layer's validation that need no context (tests/test_moving12_gpu.py then holds the device against the references)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT, converged

import moving12_oracle as mo
import srbnmpc
from srbnmpc import srb12

NEW_NAMES = ("srb12_solve_batch_moving", "srb12_solve_batch_moving_device", "srb12_obstacles_advance_device",
             "srb12_rollout_moving_device")
# agents whose X moves by more than 1e-3 between the static and the moving oracle answer at vmax = 1, and the largest
# such move, measured with the oracle alone
MOVED = {mo.SHAPES0[0]: (13, 0.155), mo.SHAPES0[1]: (5, 0.020), mo.SHAPES0[2]: (10, 0.269), mo.SHAPES0[3]: (7, 0.158)}
# the smallest run's closed loop in the moving world: smallest and median min_d_obs, aware and unaware
LOOP = {mo.RUNS0[2]: ((0.1514, 0.3214), (0.1514, 0.3192)), mo.RUNS0[0]: ((0.0988, 0.5090), (0.0781, 0.5090))}


# ================================================================================== the references
@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_reference_with_a_zero_table_is_the_static_oracle_bitwise(shape):
    R = mo.reference(shape)
    b = R["b"]
    ob = b["obstacles"]
    x0 = np.array([[x[0], x[1]] for x in b["x0"]])
    assert shape[1] <= ob.shape[0] - 1
    assert np.sqrt(((x0[:, None] - ob[None]) ** 2).sum(2)).max() < 1000.0
    z = mo.solve_moving(R["p"], b, ob, np.zeros_like(ob))
    for k in ("x_qp", "x", "obj", "status", "iters"):
        assert np.array_equal(z[k], R["r0"][k]), k


@pytest.mark.parametrize("shape", mo.SHAPES0)
def test_reference_discriminates(shape):
    """Every solve against the moving table converges, and at least a third of the batch moves by more than 1e-3
    in X against the static answer: the table matters."""
    R = mo.reference(shape)
    N, Ko, A, gait, seed = shape
    assert converged(R["r"]["status"]).all(), R["r"]["status"].tolist()
    d = np.abs(R["r"]["x"][:, :12 * N] - R["r0"]["x"][:, :12 * N]).max(1)
    n, big = int((d > 1e-3).sum()), float(d.max())
    print(f"shape {shape}: {n} of {A} agents move by more than 1e-3, up to {big:.3f}")
    assert n == MOVED[shape][0] and abs(big - MOVED[shape][1]) < 1e-3
    assert 3 * n >= A


@pytest.mark.parametrize("shape", mo.SHAPES0[:3])
def test_reference_for_given_rows_agrees_with_the_batch_reference(shape):
    """solve_selected handed the snapshot rows is solve_moving up to the order of the rows inside the sums."""
    R = mo.reference(shape)
    N, Ko = shape[0], shape[1]
    sel = mo.snapshot_select(R["b"], R["b"]["obstacles"], Ko)
    r = mo.solve_selected(R["p"], R["b"], R["b"]["obstacles"], R["w"], sel)
    assert np.array_equal(r["status"], R["r"]["status"])
    assert np.abs(r["x"][:, :12 * N] - R["r"]["x"][:, :12 * N]).max() < 1e-6


@pytest.mark.parametrize("run", list(LOOP))
def test_oracle_closed_loop_in_the_moving_world(run):
    for aware, (lo, med) in zip((True, False), LOOP[run]):
        R = mo.closed_loop12_moving(run, aware)
        st = R["status"]
        assert converged(st.reshape(-1, 2)).all()
        d = R["metrics"]["min_d_obs"]
        print(f"run {run} aware {aware}: min_d_obs smallest {d.min():.4f} median {np.median(d):.4f}")
        assert abs(d.min() - lo) < 6e-4 and abs(np.median(d) - med) < 6e-4


# ================================================================================== names and layout
def test_header_declares_and_library_exports_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    L = srbnmpc.lib()
    for n in NEW_NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(L, n), n
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert L.srb_abi_version() == 6 == srbnmpc.ABI_VERSION


def test_layouts_match_the_header(tmp_path):
    structs = (("srb12_batch", srb12.Batch12), ("srb12_sim", srb12.Sim12), ("srb12_plans", srb12.Plans12),
               ("srb_moving", srbnmpc.Moving))
    body = ""
    for name, cls in structs:
        body += f'  printf("%zu\\n", sizeof({name}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\nint main(void) {\n' + body +
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for name, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
    assert [f for f, _ in srbnmpc.Moving._fields_] == ["struct_size", "obs_vel", "horizon_selection", "obstacles"]
    assert ctypes.sizeof(srbnmpc.Moving) == 32 and ctypes.sizeof(srb12.Plans12) == 40


# ================================================================================== refusals without a context
def test_refusals_that_need_no_gpu():
    """The refusals of srb_moving are made by name (SRB_ERR_ARG = -1) with a NULL context: nothing is launched."""
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    d, e = np.zeros(64), np.zeros(64)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    M, B = srbnmpc.Moving, srb12.Batch12
    sim = srb12.Sim12(); sim.goal = ptr(d)
    calls = (lambda b, mv: lib.srb12_solve_batch_moving(None, 1, ctypes.byref(b), None, ctypes.byref(mv)),
             lambda b, mv: lib.srb12_solve_batch_moving_device(None, 1, ctypes.byref(b), None, ctypes.byref(mv), None),
             lambda b, mv: lib.srb12_rollout_moving_device(None, 1, ctypes.byref(b), ctypes.byref(sim), None,
                                                           ctypes.byref(mv), 1, None))
    for i, fn in enumerate(calls):
        for bad in (0, ctypes.sizeof(M) - 8, ctypes.sizeof(M) + 8, ctypes.sizeof(B)):
            mv = M(); mv.struct_size = bad
            assert fn(B(), mv) == -1 and "srb_moving.struct_size" in err()
        b = B(); b.struct_size += 8
        assert fn(b, M()) == -1 and "srb12_batch.struct_size" in err()
        for bad in (2, -1):
            mv = M(ptr(d), bad, None)
            assert fn(B(), mv) == -1 and "srb_moving.horizon_selection: 0" in err()
        assert fn(B(), M(None, 1, None)) == -1 and "horizon_selection = 1 needs obs_vel" in err()
        b = B(); b.obstacles_version = 3
        assert fn(b, M(ptr(d), 0, None)) == -1 and "obstacles_version != 0" in err()
        if i == 2:
            b = B(); b.obstacles = ptr(e)
            assert fn(b, M(ptr(d), 0, None)) == -1 and "srb12_rollout_moving_device: srb_moving.obstacles missing" in err()
            assert fn(b, M(ptr(d), 0, ptr(d))) == -1 and "is not srb12_batch.obstacles" in err()
            assert fn(b, M(ptr(d), 0, ptr(e))) == -1 and "null argument" in err()
        else:
            assert fn(B(), M(ptr(d), 1, None)) == -1 and "null argument" in err()
        assert fn(B(), M()) == -1 and "null argument" in err()          # a table-less srb_moving: the entry extended
    assert lib.srb12_obstacles_advance_device(None, 1, ptr(d), ptr(e), None) == -1 and "null ctx" in err()


def test_python_layer_validates_by_name_without_a_context():
    """obs_vel / obs_horizon are checked before the library (or the context) is touched: a Solver12 that was never
    created serves."""
    s = srb12.Solver12.__new__(srb12.Solver12)
    s.params, s._scenes, s._h = srb12.default_params(10, K_obs=1, K_nbr=0), (0, 0), None
    s.max_agents, s.device = 8, 0
    A, N, n_obs = 4, 10, 5
    x0, xref, foot = np.zeros((A, 12)), np.zeros((A, N, 12)), np.zeros((A, N, 4, 3))
    contact, ob = np.zeros((A, N, 4), np.int32), np.zeros((n_obs, 2))
    for bad in (np.zeros((n_obs, 2), np.float32), np.zeros((n_obs, 3)), np.zeros((n_obs + 1, 2)),
                np.zeros((n_obs, 4))[:, ::2], [[0.0, 0.0]] * n_obs):
        with pytest.raises(ValueError, match="obs_vel must be a contiguous float64 array"):
            s.solve(x0, xref, foot, contact, ob, obs_vel=bad)
    q = srb12.Solver12.__new__(srb12.Solver12)
    q.params, q._scenes, q._h = srb12.default_params(10, K_obs=1, K_nbr=0, use_nlp=0), (0, 0), None
    with pytest.raises(ValueError, match="QP-only solve has no obstacle rows"):
        q.solve(x0, xref, foot, contact, ob, obs_vel=np.zeros((n_obs, 2)))
    torch = pytest.importorskip("torch")
    t = lambda a: torch.as_tensor(a)
    out = dict(x=t(np.zeros((A, 241))), obj=t(np.zeros(A)), status=t(np.zeros((A, 2), np.int32)),
               iters=t(np.zeros((A, 2), np.int32)))
    args = (t(x0), t(xref), t(foot), t(contact), t(ob), None)
    for bad in (torch.zeros(n_obs, 2, dtype=torch.float32), torch.zeros(n_obs + 1, 2, dtype=torch.float64),
                torch.zeros(n_obs, 4, dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="obs_vel must be"):
            s.solve_device(*args, out, obs_vel=bad)
        with pytest.raises(ValueError, match="obs_vel must be"):
            s.solve_coupled_device(*args, dict(out, plan=torch.zeros(A, N, 2, dtype=torch.float64)), outer=1, obs_vel=bad)
        with pytest.raises(ValueError, match="obs_vel must be"):
            s.advance_obstacles_device(t(ob), bad)
    with pytest.raises(ValueError, match="obstacles must be"):
        s.advance_obstacles_device(torch.zeros(n_obs, 3, dtype=torch.float64), torch.zeros(n_obs, 2, dtype=torch.float64))
    import inspect
    for fn in (srb12.Solver12.solve, srb12.Solver12.solve_device, srb12.Solver12.solve_coupled_device,
               srb12.Rollout12.__init__):
        assert {"obs_vel", "obs_horizon"} <= set(inspect.signature(fn).parameters), fn
