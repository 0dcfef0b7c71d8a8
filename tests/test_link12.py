"""The degraded neighbour link of the SRB-12 mode, the part that needs no GPU: workload.cross_goals, the refusals by
name through the loaded library, the argument checks of Rollout12(link=...) (the one copy in rollout._RolloutBase, on
CPU tensors), the restatement of the selection with an own plan (link12_oracle.select_own) and the start geometry of
the closed-loop test on the CPU oracle alone.  The GPU half is test_link12_gpu.py."""
import ctypes
import types

import numpy as np
import pytest

import link12_oracle as l12
import srbnmpc
import test_link
from srbnmpc import rollout, srb12, workload
from test_nbr_plan import brute_force, crossing_tables

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
NEW_SYMBOLS = ("srb12_link_update_device", "srb12_solve_batch_link_device", "srb12_rollout_link_device")
X_TOL = 1e-6                                                # tests/test_srb12.py


# ---------------------------------------------------------------- workload.cross_goals
@pytest.mark.parametrize("make,team,S", [("lip", 8, 3), ("srb12", 4, 5), ("lip", 2, 2), ("srb12", 3, 1)])
def test_cross_goals_is_one_derangement_per_scene_and_reproducible(make, team, S):
    sc = (workload.make_scenes(S, team, 4, 2, seed=7, n_obs=3) if make == "lip" else
          workload.make_scenes12(S, team, 4, "trot", seed=7, n_obs=3))
    starts = np.array(sc["nbr_state"][:, :2])
    before = starts.copy()
    g = workload.cross_goals(starts, team, seed=5)
    assert g.shape == (S * team, 2) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(starts, before)                       # the input is not modified
    perms = []
    for s in range(S):
        mine, got = starts[s * team:(s + 1) * team], g[s * team:(s + 1) * team]
        perm = [int(np.nonzero((mine == row).all(1))[0][0]) for row in got]   # a row of this scene, found exactly
        assert sorted(perm) == list(range(team))                # a permutation within the scene: nobody shares a goal
        assert all(perm[i] != i for i in range(team))           # without a fixed point: nobody keeps one
        perms.append(perm)
    assert all(p == perms[0] for p in perms)                    # the same for every scene
    assert np.array_equal(g, workload.cross_goals(starts, team, seed=5))
    if team >= 4:                                               # (2 agents have one derangement, 3 have two)
        assert any(not np.array_equal(g, workload.cross_goals(starts, team, seed=q)) for q in range(6, 16))
    # replicas of a scene stay replicas
    rep = workload.replicate_scenes(sc, 3)
    gr = workload.cross_goals(rep["nbr_state"][:, :2], team, seed=5)
    assert np.array_equal(gr, np.tile(g, (3, 1)))


def test_cross_goals_refuses_by_name_what_it_cannot_cross():
    sc = workload.make_scenes(2, 4, 4, 2, seed=1, n_obs=2)
    with pytest.raises(ValueError, match="two agents with one goal"):
        workload.cross_goals(sc["goal"], 4)                     # make_scenes: one goal a team
    with pytest.raises(ValueError, match="not whole scenes"):
        workload.cross_goals(sc["nbr_state"][:7, :2], 4)
    with pytest.raises(ValueError, match="not whole scenes"):
        workload.cross_goals(sc["nbr_state"][:, :2], 1)
    with pytest.raises(ValueError, match=r"goals must be \[n\]\[2\]"):
        workload.cross_goals(sc["nbr_state"], 4)
    # the other draws of the module are what they were
    assert np.array_equal(sc["x0"], workload.make_scenes(2, 4, 4, 2, seed=1, n_obs=2)["x0"])


# ---------------------------------------------------------------- the C ABI without a context
def test_symbols_and_the_abi_version_stay():
    lib = srb12._lib()
    for name in NEW_SYMBOLS + test_link.NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.srb_abi_version() == 6


def _sim12(keep, n, N):
    f = lambda *sh: keep.setdefault(len(keep), np.zeros(sh))
    sim = srb12.Sim12()
    sim.goal, sim.last_state = f(n, 2).ctypes.data_as(_dp), f(n, 4).ctypes.data_as(_dp)
    return sim


def test_refusals_by_name_without_a_context():
    """Every refusal of srb_link that needs no context, through srb12_link_update_device and
    srb12_rollout_link_device (test_link.refusal_cases: 3 rows, N = 4), and those of the own plan through
    srb12_solve_batch_link_device.  A struct that passes gets as far as the missing context."""
    lib = srb12._lib()
    keep = {}
    err = lambda: lib.srb_last_error().decode()
    n, N = 3, 4
    last, table, plan = np.zeros((n, 4)), np.zeros((n, N, 2)), np.zeros((n, N, 2))
    lp, tp, pp = (a.ctypes.data_as(_dp) for a in (last, table, plan))
    for link, word, needs_plan in test_link.refusal_cases(keep):
        assert lib.srb12_link_update_device(None, n, ctypes.byref(link), lp, tp, 1, 0, None) == -1 and word in err(), (word, err())
        if needs_plan:
            assert lib.srb12_link_update_device(None, n, ctypes.byref(link), lp, None, 1, 0, None) == -1
            assert "null argument" in err(), err()
        sim = _sim12(keep, n, N)
        sim.last_state = lp
        pl = srb12.Plans12(None, pp, 0, tp)
        rc = lib.srb12_rollout_link_device(None, n, ctypes.byref(srb12.Batch12()), ctypes.byref(sim), ctypes.byref(pl),
                                           None, None, None, None, ctypes.byref(link), 1, None)
        assert rc == -1 and word in err(), (word, err())
        if needs_plan:                                         # plans off: the plan buffers may be absent
            rc = lib.srb12_rollout_link_device(None, n, ctypes.byref(srb12.Batch12()), ctypes.byref(sim), None, None, None,
                                               None, None, ctypes.byref(link), 1, None)
            assert rc == -1 and "null argument" in err(), err()
    over = test_link.make_link(keep, seen_state=ctypes.cast(ctypes.c_void_p(last.ctypes.data + 32), _dp))
    assert lib.srb12_link_update_device(None, n, ctypes.byref(over), lp, None, 1, 0, None) == -1
    assert "srb_link.seen_state overlaps last_state" in err()
    sim = _sim12(keep, n, N)
    sim.last_state = lp
    assert lib.srb12_rollout_link_device(None, n, ctypes.byref(srb12.Batch12()), ctypes.byref(sim), None, None, None, None,
                                         None, ctypes.byref(over), 1, None) == -1
    assert "srb_link.seen_state overlaps last_state" in err()
    assert lib.srb12_link_update_device(None, n, ctypes.byref(test_link.make_link(keep)), lp, None, 1, 2, None) == -1
    assert "cycle precedes c_first" in err()
    for link in (test_link.make_link(keep), test_link.make_link(keep, delay=None), srbnmpc.Link()):
        assert lib.srb12_link_update_device(None, n, ctypes.byref(link), lp, tp, 1, 0, None) == -1
        assert "null argument" in err(), err()
    # the struct-size refusal of srb12_sim comes first, as in every srb12_sim entry point
    bad = srb12.Sim12()
    bad.struct_size -= 8
    assert lib.srb12_rollout_link_device(None, n, ctypes.byref(srb12.Batch12()), ctypes.byref(bad), None, None, None, None,
                                         None, ctypes.byref(test_link.make_link(keep, max_delay=17)), 1, None) == -1
    assert "srb12_sim.struct_size" in err()
    # ---- the own plan of the selection
    own = np.zeros((n, N, 2))
    op = own.ctypes.data_as(_dp)
    b = srb12.Batch12()
    b.nbr_state, b.n_all = lp, n
    solve = lambda pl, ag=None: lib.srb12_solve_batch_link_device(None, n, ctypes.byref(b), pl, None, None, ag, op, None)
    for pl in (None, ctypes.byref(srb12.Plans12(tp, pp, 0, None))):
        assert solve(pl) == -1 and "own_plan needs srb12_plans.plan_selection = 1" in err(), err()
    assert solve(ctypes.byref(srb12.Plans12(tp, op, 1, None))) == -1 and "own_plan overlaps srb12_plans.plan" in err()
    rad = np.full(n, 0.7)
    ag = srbnmpc.AgentSizes(rad.ctypes.data_as(_dp), None, None, 1, None)
    assert solve(ctypes.byref(srb12.Plans12(tp, pp, 1, None)), ctypes.byref(ag)) == -1
    assert "own_plan with srb_agent_sizes.clearance_selection = 1" in err()
    assert solve(ctypes.byref(srb12.Plans12(tp, pp, 1, None))) == -1 and "null argument" in err(), err()
    # without an own plan the entry point refuses what srb12_solve_batch_agents_device refuses, in its words
    for f, tail in ((lib.srb12_solve_batch_link_device, (None, None)), (lib.srb12_solve_batch_agents_device, (None,))):
        assert f(None, n, ctypes.byref(b), ctypes.byref(srb12.Plans12(None, pp, 1, None)), None, None, None, *tail) == -1
        assert "plan_selection = 1 needs nbr_plan" in err()


# ---------------------------------------------------------------- Rollout12(link=...): the shared checks
def _stub(cls, N=4, plans=True):
    """An object of the rollout class with what _set_link reads, on the CPU (no context is created)."""
    torch = pytest.importorskip("torch")
    r = object.__new__(cls)
    r.device, r.plans = torch.device("cpu"), plans
    r.solver = types.SimpleNamespace(params=types.SimpleNamespace(N=N))
    return torch, r


def test_both_modes_share_one_copy_of_the_link_checks():
    base = rollout._RolloutBase
    for cls in (srbnmpc.Rollout, srb12.Rollout12):
        assert cls._set_link is base._set_link and cls._link is base._link
        assert "_set_link" not in vars(cls) and "_link" not in vars(cls)
    assert "link" in srb12.Rollout12.__init__.__code__.co_varnames
    assert "own_plan" in srb12.Solver12.solve_device.__code__.co_varnames


@pytest.mark.parametrize("cls", [srbnmpc.Rollout, srb12.Rollout12])
def test_rollout_link_argument_checks_by_name(cls):
    torch, r = _stub(cls)
    n = 6
    i4 = lambda v: torch.full((n,), v, dtype=torch.int32)
    f8 = lambda v, rows=n: torch.full((rows,), v, dtype=torch.float64)
    M = srbnmpc.LinkModel
    for link, word in ((dict(delay=None), "link must be a srbnmpc.LinkModel"),
                       (M(seed=-1), "seed must be 0"), (M(seed=1 << 64), "seed must be 0"),
                       (M(delay=i4(17)), "delay must be 0 .. 16"), (M(delay=i4(-1)), "delay must be 0 .. 16"),
                       (M(delay=f8(1.0)), "link: delay must be a contiguous torch.int32"),
                       (M(drop=f8(0.1, n + 1)), "link: drop must be a contiguous"),
                       (M(drop=f8(1.5)), "drop must be <= 1"), (M(drop=f8(-0.1)), "drop must be >= 0"),
                       (M(noise_p=f8(float("nan"))), "noise_p must be finite"),
                       (M(noise_v=f8(-1.0)), "noise_v must be >= 0")):
        with pytest.raises(ValueError, match=word):
            r._set_link(link, n)
    r._set_link(None, n)
    assert r.link is None and r.seen_state is None
    r._set_link(M(seed=3), n)                                   # nothing set: the plain rollout
    assert r.link is None and r.seen_state is None and r.seen_plan is None and r.age_log is None
    r._set_link(M(seed=3, delay=i4(2), noise_p=f8(0.03), extrapolate=True), n)
    assert r.link is not None and r._link_delay == 2 and r._link_extrapolate == 1 and r._link_rows == n
    assert tuple(r._ring_state.shape) == (3, n, 4) and tuple(r._ring_plan.shape) == (3, n, 4, 2)
    assert tuple(r.seen_state.shape) == (n, 4) and tuple(r.seen_plan.shape) == (n, 4, 2)
    ln = r._link()
    assert ln.struct_size == ctypes.sizeof(srbnmpc.Link) and ln.max_delay == 2 and ln.extrapolate == 1 and ln.seed == 3
    assert not ln.drop and not ln.noise_v and not ln.age_log and ln.seen_plan
    _, q = _stub(cls, plans=False)
    q._set_link(M(drop=f8(0.2)), n)
    assert q.seen_plan is None and q._ring_plan is None and q._link_delay == 0 and not q._link().ring_plan


def test_rollout12_still_refuses_the_lip_plant_arguments_and_takes_plan_selection_with_a_link():
    with pytest.raises(ValueError, match="Rollout12: kick_v is not available"):
        srb12.Rollout12(None, None, kick_v=np.zeros(3), link=srbnmpc.LinkModel())
    # (no refusal of plan_selection under a link in the SRB-12 layer: the word appears in the LIP refusal only)
    import inspect
    assert "plan_selection" not in inspect.getsource(rollout._RolloutBase._set_link)


# ---------------------------------------------------------------- the restatement of the selection with an own plan
@pytest.mark.parametrize("n_all,N,Kn,scene", [(2, 10, 2, 0), (5, 4, 2, 0), (40, 10, 8, 0), (12, 10, 3, 4)])
def test_own_plan_equal_to_the_table_row_is_the_plain_restatement(n_all, N, Kn, scene):
    x0, nbr, plan = crossing_tables(n_all, N, seed=50 + n_all)
    kn = min(Kn, (scene or n_all) - 1)
    got = l12.select_own(x0, nbr, plan, plan.copy(), kn, scene_agents=scene)
    none = l12.select_own(x0, nbr, plan, None, kn, scene_agents=scene)
    if scene:
        want = np.concatenate([brute_force(x0[i:i + scene], nbr[i:i + scene], plan[i:i + scene], kn) + i
                               for i in range(0, n_all, scene)])
    else:
        want = brute_force(x0, nbr, plan, kn)
    assert np.array_equal(got, want) and np.array_equal(none, want)
    # a shard: the own plans are indexed by the local agent
    if n_all == 40:
        part = l12.select_own(x0[13:29], nbr, plan, plan[13:29].copy(), kn, lo=13)
        assert np.array_equal(part, want[13:29])
        # ... and another own plan changes columns of its agent alone
        own = plan.copy()
        own[7] += 25.0
        moved = l12.select_own(x0, nbr, plan, own, kn)
        assert not np.array_equal(moved[7], want[7]) and np.array_equal(np.delete(moved, 7, 0), np.delete(want, 7, 0))


# ---------------------------------------------------------------- the closed-loop test's geometry, on the oracle alone
@pytest.mark.parametrize("extrapolate", [0, 1])
def test_the_head_on_start_meets_the_cap_and_the_link_matters_on_the_oracle_alone(extrapolate):
    """What test_link12_gpu's closed-loop test asks of the device, asked of the CPU oracle first: at least 90 % of the
    agent-cycles converge, some answer on the true tables is further than 100 X_TOL from the one on the perceived
    tables, and every plan table of an N = 4 rollout is a line (link12_oracle.linear_rows)."""
    A, N, gait, seed, T, Ko, Kn = l12.LOOP
    compared, matters, closest, err = l12.oracle_loop(extrapolate, X_TOL)
    print(f"extrapolate {extrapolate}: {compared}/{T * A} agent-cycles converged, {matters} moved by the link, closest "
          f"pair {closest:.3f} m, tables within {err:.1e} of their lines")
    assert compared >= 0.9 * T * A and matters >= 1 and err < l12.LINE_TOL
    assert closest < np.sqrt(workload.EPS_NBR)                 # the inter-agent rows are active
