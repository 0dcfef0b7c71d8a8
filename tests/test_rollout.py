"""CPU tests of the closed-loop rollout: the numpy restatement of the rollout kernels (tests/sim_oracle.py)
against the pieces it restates -- workload.make_batch's reference and footholds, dist.shift_plans -- its arrival
cases, the srb_sim layout and the refusals that need no GPU, and the oracle-only closed loop on the four runs of
sim_oracle.RUNS, which must stay OPTIMAL in every cycle (tests/test_rollout_gpu.py then holds the device closed
loop against the same restatement)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT, converged

import plan_oracle
import sim_oracle
import srbnmpc
from srbnmpc import workload

TS = workload.TS


def _workload_phase(A, seed):
    """The gait phase make_batch draws per agent (it does not return it): the same generator, the same draws."""
    rng = np.random.default_rng(seed)
    rng.uniform(0, 1, A); rng.uniform(0, 1, A); rng.uniform(0, 0.3, (A, 1)); rng.uniform(-0.05, 0.05, (A, 2))
    return rng.integers(0, 4, A)


@pytest.mark.parametrize("N,C", [(10, 2), (4, 4), (6, 2)])
def test_restatement_agrees_with_make_batch_where_the_rules_coincide(N, C):
    """From make_batch's own start positions, far from the goal, cycle 0: the same reference for every agent and
    the same footholds for the agents make_batch gave gait phase 0 (the rollout's domains start at the cycle).
    The two group the products differently (make_batch: ((d v) Ts) (k + 1)), so equal to round-off, not bitwise."""
    A, seed = 64, 3
    b = workload.make_batch(A, N, C, seed=seed)
    goal = np.tile(workload.GOAL * np.array([workload.arena_scale(A), 1.0]), (A, 1))
    far = np.hypot(goal[:, 0] - b["x0"][:, 0], goal[:, 1] - b["x0"][:, 2]) > workload.VREF * TS * N
    assert far.all()
    r = sim_oracle.advance(N, C, TS, b["x0"], goal, workload.VREF, 0)
    assert np.array_equal(r["x0"], b["x0"]) and np.array_equal(r["last_state"], b["nbr_state"])
    np.testing.assert_allclose(r["ref"], b["ref"], rtol=1e-13, atol=1e-14)
    ph0 = _workload_phase(A, seed) == 0
    assert ph0.sum() >= 8
    np.testing.assert_allclose(r["foot"][ph0], b["foot"][ph0], rtol=1e-13, atol=1e-14)
    # the parity flips the diagonal: cycle 1 (or phase 1) stands on the legs cycle 0 swings
    r1 = sim_oracle.advance(N, C, TS, b["x0"], goal, workload.VREF, 1)
    r1p = sim_oracle.advance(N, C, TS, b["x0"], goal, workload.VREF, 0, phase=np.ones(A, np.int32))
    assert np.array_equal(r1["foot"], r1p["foot"]) and np.array_equal(r1["ref"], r["ref"])
    if C == 2:
        assert not np.array_equal(r1["foot"], r["foot"])
        if N > 4:                                          # the second domain of cycle 0 has cycle 1's legs
            np.testing.assert_allclose(r1["foot"][:, 0] - r1["foot"][:, 0, :, :1], r["foot"][:, 4] - r["foot"][:, 4, :, :1],
                                       atol=1e-12)
    else:
        assert np.array_equal(r1["foot"], r["foot"])


@pytest.mark.parametrize("N", [4, 10])
def test_shift_equals_shift_plans_bitwise(N):
    torch = pytest.importorskip("torch")
    from srbnmpc import dist as sdist
    rng = np.random.default_rng(N)
    p = srbnmpc.default_params(N, 2)
    x = rng.normal(size=(9, p.nv)) * np.array([1.0, 3.0, 1e-3])[rng.integers(0, 3, (9, 1))]
    want = sdist.shift_plans(torch.from_numpy(plan_oracle.plans_of(p, x)), 4).numpy()
    assert np.array_equal(sim_oracle.shift4(N, x), want)
    assert np.array_equal(sim_oracle.next_state(x), x[:, 12:16])


def test_arrival_cases():
    """dist = 0: a standing reference and the stance around the agent, no NaN.  dist < vref Ts N: the line ends
    at the goal and never beyond it."""
    N, C = 10, 2
    state = np.array([[1.5, 0.0, -0.25, 0.0], [2.0, 0.0, 1.0, 0.0], [0.0, 0.1, 0.0, 0.0]])
    goal = np.array([[1.5, -0.25], [2.03, 1.02], [10.0, 0.0]])
    r = sim_oracle.advance(N, C, TS, state, goal, workload.VREF, 0)
    assert np.isfinite(r["ref"]).all() and np.isfinite(r["foot"]).all()
    ref = r["ref"].reshape(3, N, 4)
    assert np.array_equal(ref[0], np.tile([1.5, 0.0, -0.25, 0.0], (N, 1)))
    assert np.array_equal(r["foot"][0, 0], sim_oracle.STANCE[[0, 3]].T + np.array([[1.5], [-0.25]]))
    assert np.array_equal(r["foot"][0, 0], r["foot"][0, 3]) and np.array_equal(r["foot"][0, 8], r["foot"][0, 9])
    d = np.hypot(0.03, 0.02)
    assert d < workload.VREF * TS * N
    np.testing.assert_allclose(ref[1, -1, [0, 2]], goal[1], rtol=0, atol=1e-15)
    # (goal - position cancels at magnitude 2: relative round-off 2.2e-16 * 2 / 0.03 = 1.5e-14 in dist)
    assert np.hypot(*(ref[1, -1, [0, 2]] - state[1, [0, 2]])) <= d * (1 + 1e-13)
    np.testing.assert_allclose(np.hypot(ref[1, 0, 1], ref[1, 0, 3]), d / (TS * N), rtol=1e-13)
    step = np.diff(ref[1, :, 0])
    assert (step > 0).all()
    np.testing.assert_allclose(np.hypot(ref[2, :, 1], ref[2, :, 3]), workload.VREF, rtol=1e-15)   # far: the cap


def test_metrics_restatement():
    """Nearest rows, the NaN and empty-table rules, the self row, the running minima and the first crossing."""
    st = np.array([[0.0, 0, 0.0, 0], [3.0, 0, 4.0, 0], [1.0, 0, 0.0, 0]])
    nbr = np.stack([st[:, 0], st[:, 2], st[:, 1], st[:, 3]], 1)
    obs = np.array([[0.0, 0.4], [np.nan, 0.0], [3.0, 4.75]])
    m = sim_oracle.Metrics(2).update(2, st, obs, nbr)
    assert m.d_obs.tolist() == [0.4, 0.75, np.sqrt(1.0 * 1.0 + 0.4 * 0.4)] and m.d_agent.tolist() == [1.0, np.sqrt(20.0), 1.0]
    assert m.fail_cycle.tolist() == [2, -1, -1] and m.distance_to_fail.tolist() == [0.0, 0.0, 0.0]
    st2 = st.copy(); st2[1, 2] = 4.5; st2[0, 0] = 5.0
    nbr2 = np.stack([st2[:, 0], st2[:, 2], st2[:, 1], st2[:, 3]], 1)
    m.update(3, st2, obs, nbr2)
    assert m.fail_cycle.tolist() == [2, 3, -1] and m.distance_to_fail.tolist() == [0.0, np.sqrt(3.0 * 3.0 + 4.5 * 4.5), 0.0]
    assert m.min_d_obs[0] == 0.4 and m.d_obs[0] > 0.4 and m.min_d_obs[1] == 0.25
    e = sim_oracle.Metrics(0).update(0, st, None, nbr[:1], agent_offset=0)
    assert np.isinf(e.d_obs).all() and np.isinf(e.d_agent[0]) and e.d_agent[2] == 1.0 and (e.fail_cycle == -1).all()


def test_sim_layout_matches_the_header(tmp_path):
    """sizeof(srb_sim) and every member's offset, from the system C compiler, against the ctypes mirror; the ABI
    version is still 6 (entry points were added, no layout changed)."""
    names = [f for f, _ in srbnmpc.Sim._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(srb_sim), sizeof(srb_batch));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(srb_sim, {n}));\n' for n in names) +
                   '  printf("%d\\n", SRB_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = srbnmpc.Sim
    assert got[0] == ctypes.sizeof(S) and got[1] == ctypes.sizeof(srbnmpc.Batch)
    assert got[2:-1] == [getattr(S, n).offset for n in names]
    assert got[-1] == 6 == srbnmpc.lib().srb_abi_version() == srbnmpc.ABI_VERSION
    assert S().struct_size == ctypes.sizeof(S) and names[0] == "struct_size"


def test_refusals_that_need_no_gpu():
    """The layout check, the missing goal and the missing x are refused by name before a context is looked at."""
    lib = srbnmpc.lib()
    err = lambda: lib.srb_last_error().decode()
    d = np.zeros(8)
    ptr = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for fn in (lib.srb_sim_advance_device, lib.srb_sim_metrics_device):
        for bad in (0, ctypes.sizeof(srbnmpc.Sim) - 8, ctypes.sizeof(srbnmpc.Sim) + 8, ctypes.sizeof(srbnmpc.Batch)):
            s = srbnmpc.Sim(); s.struct_size = bad
            assert fn(None, 1, ctypes.byref(s), 0, None) == -1 and "srb_sim.struct_size" in err()
        assert fn(None, 1, None, 0, None) == -1 and "null argument" in err()
    s = srbnmpc.Sim()
    assert lib.srb_sim_advance_device(None, 1, ctypes.byref(s), 0, None) == -1 and "goal" in err()
    s.goal = ptr
    assert lib.srb_sim_advance_device(None, 1, ctypes.byref(s), 1, None) == -1 and "srb_sim.x" in err()
    s.c_first = 1
    assert lib.srb_sim_advance_device(None, 1, ctypes.byref(s), 0, None) == -1 and "c_first" in err()
    assert lib.srb_sim_advance_device(None, 1, ctypes.byref(s), 1, None) == -1 and "null argument" in err()
    assert lib.srb_sim_metrics_device(None, 1, ctypes.byref(s), 1, None) == -1 and "null argument" in err()
    # the driver: both layouts, then the goal
    b, s = srbnmpc.Batch(), srbnmpc.Sim()
    b.struct_size += 8
    assert lib.srb_rollout_device(None, 1, ctypes.byref(b), ctypes.byref(s), 1, None) == -1 and "srb_batch.struct_size" in err()
    b = srbnmpc.Batch(); s.struct_size -= 8
    assert lib.srb_rollout_device(None, 1, ctypes.byref(b), ctypes.byref(s), 1, None) == -1 and "srb_sim.struct_size" in err()
    s = srbnmpc.Sim()
    assert lib.srb_rollout_device(None, 1, ctypes.byref(b), ctypes.byref(s), 1, None) == -1 and "goal" in err()
    s.goal = ptr
    assert lib.srb_rollout_device(None, 1, ctypes.byref(b), ctypes.byref(s), 1, None) == -1 and "null argument" in err()


@pytest.mark.parametrize("run", sim_oracle.RUNS)
def test_oracle_closed_loop_stays_optimal(run):
    """The restatement in closed loop with plan_oracle.solve: every agent converges in every cycle (QP stage
    QP_WARM, NLP OPTIMAL), the arrival agents included, and the runs reach fail_cycle in all three states --
    inside 0.5 m from the start, crossing later, never."""
    R = sim_oracle.closed_loop(run)
    A, N, C, Ko, Kn, T, seed, plans = run
    assert R["status"].shape == (T, A, 2)
    assert converged(R["status"].reshape(-1, 2)).all(), np.argwhere(~converged(R["status"].reshape(-1, 2)))
    assert (R["status"][:, :, 0] == srbnmpc.QP_WARM).all() and (R["status"][:, :, 1] == 0).all()
    fc = R["metrics"]["fail_cycle"]
    print(f"run {run}: fail_cycle {fc.tolist()}, min_d_agent {R['metrics']['min_d_agent'].min():.4f}, "
          f"min_d_obs {R['metrics']['min_d_obs'].min():.4f}")
    if (A, N) == (16, 10):
        assert 5 <= (fc == 0).sum() <= 6 and (fc < 0).any()
    if (A, N) == (12, 4):
        assert (fc == 5).sum() == 1 and (fc[fc > 0] == 5).all()
    # the arrival agents keep a finite, standing or arriving reference and stay solvable (asserted above); how far
    # the trot's alternating support lets them sway is reported, not asserted
    sway = np.hypot(*(R["traj"][:, :2, [0, 2]] - R["goal"][None, :2]).transpose(2, 0, 1)).max(0)
    print(f"  largest distance from the goal, agents 0 and 1: {sway[0]:.4f} {sway[1]:.4f} m")
    assert np.isfinite(R["traj"]).all()
