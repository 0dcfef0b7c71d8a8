"""The disturbed plant of the SRB-12 rollout (srb12_plant), the part that needs no GPU: the roll of
plant12_oracle.py against oracle.dynamics12, its draws against plant_oracle's, the struct's layout, the refusals by
name of the C ABI and of srb12.Plant12, and the workload helper.  The GPU half is test_plant12_gpu.py.

The roll's tolerance (ROLL_K, roll_bound): one step is, per component, a sum of at most 17 terms (the identity, three
entries of A, twelve of B, c), so its rounding error is within 17 u of the sum S of the terms' magnitudes
(u = 2^-53); a term of B carries 7 more roundings (three products, two sums and the factor Ts inside W, the product
with f) and the error of Iw^-1: 16 roundings in T = Rz Ib, Iw = T Rz', the cofactors and the reciprocal, times the
condition number of I_b (0.0647 / 0.0168 = 3.9, taken as 4), and twice that of cos / sin, one ulp apart between libm
and numpy, on the same route (2 * 2 * 4).  17 + 7 + 64 + 16 = 104 roundings of relative size u on terms that sum to S:
one step agrees within 104 u S.  Over four steps (at_state 0, where the matrices of all four come from one call and
the comparison is at the end) an error passes through |A_k|_inf <= 1 + Ts sqrt2, so the end state agrees within
104 u S (1 + a + a^2 + a^3).  With at_state 1 every step is compared on its own, from the restatement's state.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import oracle
import plant12_oracle as p12
import plant_oracle
import sim12_oracle
import srbnmpc
from srbnmpc import srb12, workload

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
NEW_SYMBOLS = ("srb12_sim_advance_plant_device", "srb12_rollout_plant_device")
FIELDS = ("struct_size", "seed", "kick_v", "kick_p", "kick_w", "plant_mass", "plant_inertia", "at_state", "n_push",
          "push_cycle", "push_agent", "push_dv", "dist_log")
U_ROUND = 2.0 ** -53
ROLL_K = 104


def roll_case(A, N, gait, seed):
    """Random states with |yaw| up to pi, the advance's xref / foot / contact for them, and a decision vector whose
    forces are of standing size (a quarter to the whole weight per leg, sideways up to a third of that)."""
    rng = np.random.default_rng(seed)
    st = rng.normal(size=(A, 12)) * 0.05
    st[:, 0] = rng.uniform(0, 9, A); st[:, 1] = rng.uniform(-2, 2, A); st[:, 2] += 0.3
    st[:, 5] = rng.uniform(-np.pi, np.pi, A); st[:, 6:8] = rng.uniform(-.3, .3, (A, 2))
    st[:, 9:12] = rng.uniform(-0.5, 0.5, (A, 3))
    goal = np.tile([10.0, 0.0], (A, 1))
    phase = rng.integers(0, 4, A).astype(np.int32)
    b = sim12_oracle.advance12(N, workload.TS, st, goal, 0.27, 3, phase, gait)
    x = rng.normal(size=(A, 24 * N + 1))
    U = x[:, 12 * N:24 * N].reshape(A, N, 4, 3)
    U[..., 2] = rng.uniform(30, 120, (A, N, 4))
    U[..., :2] = rng.uniform(-40, 40, (A, N, 4, 2))
    return st, b, x


def roll_bound(A_, B_, c_, z, u, steps):
    S = (np.abs(A_) @ np.abs(z) + np.abs(B_) @ np.abs(u) + np.abs(c_)).max()
    a = 1.0 + workload.TS * np.sqrt(2.0)
    return ROLL_K * U_ROUND * S * sum(a ** k for k in range(steps))


@pytest.mark.parametrize("N,gait", [(4, "trot"), (10, "trot"), (4, "stand"), (10, "stand")])
def test_the_restated_roll_is_the_oracles_dynamics(N, gait):
    A = 6
    st, b, x = roll_case(A, N, gait, 77 + N + len(gait))
    p = oracle.params12(N)
    rng = np.random.default_rng(N)
    mass, inertia = p.mass * rng.uniform(0.85, 1.15, A), rng.uniform(0.8, 1.25, A)
    m, Ibs = p12.body_tables(p, A, 0, mass, inertia)
    U = x[:, 12 * N:24 * N].reshape(A, N, 12)
    worst = {0: (0.0, 0.0), 1: (0.0, 0.0)}
    for at_state in (0, 1):
        tr = p12.roll12(p, st, x, b["xref"], b["foot"], b["contact"], m, Ibs, bool(at_state), trace=True)
        for a in range(A):
            q = oracle.params12(N)
            q.mass = float(m[a])
            for i in range(9):
                q.Ib[i] = float(Ibs[a].reshape(9)[i])
            if not at_state:
                # one call: the model's matrices for this body, rows 0 .. 3; the roll by plain products
                Ak, Bk, ck = oracle.dynamics12(q, st[a], b["xref"][a], b["foot"][a], b["contact"][a])
                z, bound = st[a], 0.0
                for k in range(4):
                    bound = max(bound, roll_bound(Ak[k], Bk[k], ck[k], z, U[a, k], 4))
                    z = Ak[k] @ z + Bk[k] @ U[a, k] + ck[k]
                err = np.abs(tr[3][a] - z).max()
                assert err <= bound, (at_state, a, err, bound)
                worst[0] = max(worst[0], (err, bound))
            else:
                # one N = 1 call per step at the rolled state itself
                q.N = 1
                z = st[a]
                for k in range(4):
                    Ak, Bk, ck = oracle.dynamics12(q, z, np.zeros((1, 12)), b["foot"][a, k:k + 1], b["contact"][a, k:k + 1])
                    want = Ak[0] @ z + Bk[0] @ U[a, k] + ck[0]
                    bound = roll_bound(Ak[0], Bk[0], ck[0], z, U[a, k], 1)
                    err = np.abs(tr[k][a] - want).max()
                    assert err <= bound, (at_state, a, k, err, bound)
                    worst[1] = max(worst[1], (err, bound))
                    z = tr[k][a]
    print(f"N {N} {gait}: at_state 0 end |roll - A z + B u + c| {worst[0][0]:.3e} (bound {worst[0][1]:.3e}); "
          f"at_state 1 per step {worst[1][0]:.3e} (bound {worst[1][1]:.3e})")
    # a swing leg's force is not applied, and the two linearisation points give different rolls
    z0 = p12.roll12(p, st, x, b["xref"], b["foot"], b["contact"], m, Ibs, False)
    z1 = p12.roll12(p, st, x, b["xref"], b["foot"], b["contact"], m, Ibs, True)
    assert np.array_equal(z0[:, [0, 1, 2, 6, 7, 8]], z1[:, [0, 1, 2, 6, 7, 8]]) and (z0[:, 9:12] != z1[:, 9:12]).any()
    if gait == "trot":
        x2 = x.copy()
        x2[:, 12 * N:24 * N].reshape(A, N, 4, 3)[b["contact"] == 0] += 50.0
        assert np.array_equal(p12.roll12(p, st, x2, b["xref"], b["foot"], b["contact"], m, Ibs, False), z0)


def test_the_model_body_rolls_to_the_models_prediction_of_a_feasible_x():
    """With the model's mass and inertia and at_state 0 the roll is the model: an x whose X rows satisfy the equality
    rows X_k = A_k X_{k-1} + B_k U_k + c_k is reproduced to the roll's bound."""
    N, A = 4, 5
    st, b, x = roll_case(A, N, "trot", 5)
    p = oracle.params12(N)
    m, Ibs = p12.body_tables(p, A)
    U = x[:, 12 * N:24 * N].reshape(A, N, 12)
    bound = 0.0
    for a in range(A):
        Ak, Bk, ck = oracle.dynamics12(p, st[a], b["xref"][a], b["foot"][a], b["contact"][a])
        z = st[a]
        for k in range(N):
            bound = max(bound, roll_bound(Ak[k], Bk[k], ck[k], z, U[a, k], 4))
            z = Ak[k] @ z + Bk[k] @ U[a, k] + ck[k]
            x[a, 12 * k:12 * k + 12] = z
    got, d = p12.plant_state12(p, 4, st, x, b["xref"], b["foot"], b["contact"], mass=np.full(A, p.mass))
    assert (d == 0).all() and np.abs(got - sim12_oracle.next_state12(x)).max() <= bound


def test_the_draws_are_the_lip_plants_and_counter_one():
    seed, c, rows = (0x299f31d0 << 32) | 0xa4093822, 9, 7 + np.arange(40)
    u0, u1 = plant_oracle.kicks(seed, c, rows), p12.angular_kicks(seed, c, rows)
    kv, kp, kw = np.linspace(0.01, 0.1, 60), np.linspace(0.0, 0.02, 60), np.linspace(0.02, 0.3, 60)
    d = p12.disturbance12(40, c, 7, seed, kv, kp, kw)
    # counter 0: plant_oracle.plant_state's (dpx, dvx, dpy, dvy), bitwise
    x = np.zeros((40, 41))
    _, dl = plant_oracle.plant_state(10, workload.TS, 9.81, c, None, x, agent_offset=7, seed=seed, kick_v=kv, kick_p=kp)
    assert np.array_equal(d[:, [0, 6, 1, 7]], dl) and np.array_equal(d[:, 6], 0.0 + kv[rows] * u0[:, 0])
    # counter 1: Philox at (c, g, 1, 0), words 0 .. 2
    for i, g in enumerate(rows):
        w = plant_oracle.philox4x32_10(np.array([c, g, 1, 0]), np.array([0xa4093822, 0x299f31d0]))
        assert np.array_equal(u1[i], plant_oracle.uniform(w))
    assert np.array_equal(d[:, 9:12], 0.0 + kw[rows, None] * u1[:, :3]) and (d[:, [2, 3, 4, 5, 8]] == 0).all()
    assert not np.array_equal(u0, u1)
    # pushes: table order, the firing cycle only, rows outside the batch left out
    push = (np.array([c, c, c + 1, c], np.int32), np.array([9, 9, 9, 3], np.int32), np.arange(24.0).reshape(4, 6))
    dp_ = p12.disturbance12(40, c, 7, seed, None, None, None, push)
    assert np.array_equal(dp_[2, 6:12], (0.0 + push[2][0]) + push[2][1]) and not dp_[np.arange(40) != 2].any()


def test_plant12_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(FIELDS) + '\\n", sizeof(srb12_plant)'
                   + "".join(f", offsetof(srb12_plant, {n})" for n in FIELDS) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = srb12.PlantStruct12
    assert [f[0] for f in S._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in FIELDS]
    assert S().struct_size == ctypes.sizeof(S)


def test_abi_version_stays_and_the_new_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr and "typedef struct srb12_plant {" in hdr
    assert srbnmpc.lib().srb_abi_version() == 6
    assert srb12.Sim12._fields_[-1][0] == "distance_to_fail" and srbnmpc.Plant._fields_[-1][0] == "dist_log"
    for name in NEW_SYMBOLS:
        assert hasattr(srb12._lib(), name), name


def refusal_cases():
    """(keep-alive arrays, [(plant, word, needs a srb12_sim buffer missing)]) of every refusal of srb12_plant that needs
    no context: a null context reaches them (test_plant12_gpu.py repeats them on a live one)."""
    tab, ci, dv = np.ones(3), np.zeros(3, np.int32), np.zeros((3, 6))
    pt, pi, pv = tab.ctypes.data_as(_dp), ci.ctypes.data_as(_ip), dv.ctypes.data_as(_dp)
    P = srb12.PlantStruct12
    bad_size = P()
    bad_size.struct_size += 8
    cases = [(bad_size, "srb12_plant.struct_size", None),
             (P(0, pt, None, None, None, None, 0, -1, pi, pi, pv, None), "srb12_plant.n_push: 0 .. 4096", None),
             (P(0, pt, None, None, None, None, 0, 4097, pi, pi, pv, None), "srb12_plant.n_push: 0 .. 4096", None),
             (P(0, None, None, None, None, None, 0, 3, None, pi, pv, None), "srb12_plant.n_push > 0 needs push_cycle", None),
             (P(0, None, None, None, None, None, 0, 3, pi, None, pv, None), "srb12_plant.n_push > 0 needs push_cycle", None),
             (P(0, None, None, None, None, None, 0, 3, pi, pi, None, None), "srb12_plant.n_push > 0 needs push_cycle", None),
             (P(0, pt, None, None, None, None, 2, 0, None, None, None, None), "srb12_plant.at_state", None),
             (P(0, pt, None, None, None, None, -1, 0, None, None, None, None), "srb12_plant.at_state", None)]
    for missing in ("x", "xref", "foot", "contact"):
        cases += [(P(7, None, None, None, pt, None, 0, 0, None, None, None, None), "need srb12_sim.x, xref, foot", missing),
                  (P(7, None, None, None, None, pt, 0, 0, None, None, None, None), "need srb12_sim.x, xref, foot", missing),
                  (P(7, None, None, None, None, None, 1, 0, None, None, None, None), "need srb12_sim.x, xref, foot", missing)]
    return (tab, ci, dv), cases


def call_refused(lib, h, entry, plant, sim, b=None, n_agents=1):
    b = srb12.Batch12() if b is None else b
    if entry == "rollout":
        return lib.srb12_rollout_plant_device(h, n_agents, ctypes.byref(b), ctypes.byref(sim), None, None, None, None,
                                              ctypes.byref(plant), 1, None)
    return lib.srb12_sim_advance_plant_device(h, n_agents, ctypes.byref(sim), ctypes.byref(plant), sim.c_first + 1, None)


def full_sim(keep):
    """A srb12_sim whose goal, x, xref, foot and contact are set (host memory: nothing is launched without a context)."""
    sim = srb12.Sim12()
    g = np.zeros(64)
    keep.append(g)
    sim.goal = sim.x = sim.xref = sim.foot = g.ctypes.data_as(_dp)
    sim.contact = g.ctypes.data_as(_ip)
    return sim


def test_refusals_by_name_without_a_context():
    lib = srb12._lib()
    keep, cases = refusal_cases()
    keep = list(keep)
    for entry in ("advance", "rollout"):
        for plant, word, missing in cases:
            if missing and entry == "rollout":
                continue                                          # the rollout wires the buffers in and names them itself
            sim = full_sim(keep)
            if missing:
                setattr(sim, missing, None)
            if missing == "x":
                continue                                          # srb12_sim.x missing is check_sim12's own refusal, first
            assert call_refused(lib, None, entry, plant, sim) == -1, (entry, word)
            assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())
    # a struct that passes gets as far as the missing context, with the plant on or with nothing set
    for plant in (srb12.PlantStruct12(1, keep[0].ctypes.data_as(_dp), None, None, None, None, 1, 0, None, None, None, None),
                  srb12.PlantStruct12()):
        for entry in ("advance", "rollout"):
            assert call_refused(lib, None, entry, plant, full_sim(keep)) == -1
            assert "null argument" in lib.srb_last_error().decode(), (entry, lib.srb_last_error())
    # the struct-size refusal of srb12_sim comes first, as in every srb12_sim entry point
    bad = full_sim(keep)
    bad.struct_size -= 8
    assert call_refused(lib, None, "advance", cases[1][0], bad) == -1
    assert "srb12_sim.struct_size" in lib.srb_last_error().decode()


def test_plant12_refuses_by_name_and_the_old_names_still_refuse():
    import inspect
    torch = pytest.importorskip("torch")
    A = 4
    f8 = lambda v: torch.tensor(v, dtype=torch.float64)
    ok = f8([0.1] * A)
    for kw, word in ((dict(kick_v=f8([0.1, float("nan"), 0.1, 0.1])), "kick_v holds a NaN"),
                     (dict(mass=f8([1.0, float("nan"), 1.0, 1.0])), "mass holds a NaN"),
                     (dict(kick_w=f8([0.1, float("inf"), 0.1, 0.1])), "kick_w must be finite"),
                     (dict(kick_v=f8([0.1, -0.1, 0.1, 0.1])), "kick_v must be >= 0"),
                     (dict(kick_p=f8([-1e-9] * A)), "kick_p must be >= 0"),
                     (dict(kick_w=f8([-0.1] * A)), "kick_w must be >= 0"),
                     (dict(mass=f8([12.0, 0.0, 12.0, 12.0])), "mass must be > 0"),
                     (dict(inertia=f8([1.0, 1.0, -1.0, 1.0])), "inertia must be > 0"),
                     (dict(kick_v=torch.tensor([0.1] * A, dtype=torch.float32)), "kick_v must be a contiguous float64"),
                     (dict(inertia=np.ones(A)), "inertia must be a contiguous float64"),
                     (dict(mass=f8([[12.0] * A])), "mass must be a contiguous float64"),
                     (dict(seed=-1), "seed must be 0"), (dict(seed=1 << 64), "seed must be 0"),
                     (dict(pushes=(ok, ok)), "pushes must be a triple"),
                     (dict(pushes=(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                   torch.zeros((2, 2), dtype=torch.float64))), "pushes: dv"),
                     (dict(pushes=(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                                   torch.zeros((2, 6), dtype=torch.float64))), "pushes: cycle"),
                     (dict(pushes=(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                   torch.full((2, 6), float("nan"), dtype=torch.float64))), "pushes: dv holds a NaN")):
        with pytest.raises(ValueError, match=f"Plant12: {word}"):
            srb12.Plant12(**kw)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="Plant12: kick_w must have one row per agent"):
        srb12.Plant12(kick_w=f8([0.1] * (A + 1))).check(A, cpu)
    with pytest.raises(ValueError, match="Plant12: mass must be on"):
        srb12.Plant12(mass=ok).check(A, torch.device("cuda", 0))
    push = (torch.tensor([1], dtype=torch.int32), torch.tensor([A], dtype=torch.int32), torch.zeros((1, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="Plant12: pushes: agent must be a row"):
        srb12.Plant12(pushes=push).check(A, cpu)
    good = srb12.Plant12(3, ok, ok, ok, f8([12.0] * A), f8([1.0] * A), True, (push[0], torch.tensor([1], dtype=torch.int32), push[2]))
    good.check(A, cpu)
    assert good.on and good.rolls and not srb12.Plant12().on and not srb12.Plant12(seed=9).on
    assert srb12.Plant12(at_state=True).on and srb12.Plant12(kick_w=ok).on and not srb12.Plant12(kick_w=ok).rolls
    empty = (torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros((0, 6), dtype=torch.float64))
    assert not srb12.Plant12(pushes=empty).on
    # Rollout12: the LIP names still refuse, now pointing at Plant12; `plant` is in the signature and typed
    sig = inspect.signature(srb12.Rollout12.__init__).parameters
    assert "plant" in sig and sig["plant"].default is None
    for name, val in (("plant_seed", 3), ("kick_v", np.zeros(2)), ("kick_p", np.zeros(2)), ("plant_hcom", np.ones(2)),
                      ("pushes", (None, None, None))):
        assert name in sig
        with pytest.raises(ValueError, match=f"Rollout12: {name} is not available.*plant=Plant12"):
            srb12.Rollout12(None, None, **{name: val})
    with pytest.raises(ValueError, match="plant must be a srb12.Plant12"):
        srb12.Rollout12(None, None, plant=dict(kick_v=ok))


def test_plant_tables12_are_deterministic_and_leave_the_other_draws_alone():
    def others():
        out = []
        for v in (workload.make_batch(8, 10, 2, seed=5), workload.make_scenes(2, 4, 10, 2, seed=5, n_obs=5),
                  workload.make_batch12(8, 10, "trot", seed=5), workload.make_scenes12(2, 4, 10, "trot", seed=5, n_obs=5),
                  workload.agent_sizes(16, 5), workload.obstacle_sizes(20, 5), workload.obstacle_velocities(20, 5),
                  workload.plant_tables(16, 5)):
            vals = list(v.values()) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else [v]
            out += [np.array(x) for x in vals if isinstance(x, np.ndarray)]
        return out
    before = others()
    for n, seed in ((16, 5), (320, 12), (1, 0)):
        tabs = workload.plant_tables12(n, seed)
        assert len(tabs) == 5
        for v, w in zip(tabs, workload.plant_tables12(n, seed)):
            assert v.shape == (n,) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] and np.array_equal(v, w)
        kv, kp, kw, mass, inertia = tabs
        g = np.random.default_rng(500 + seed)
        assert np.array_equal(kv, g.uniform(0.02, 0.08, n)) and np.array_equal(kp, g.uniform(0.0, 0.01, n))
        assert np.array_equal(kw, g.uniform(0.02, 0.1, n))
        assert np.array_equal(mass, workload.MASS12 * g.uniform(0.85, 1.15, n))
        assert np.array_equal(inertia, g.uniform(0.8, 1.25, n))
        # the ranges the docstring states
        assert (kv >= 0.02).all() and (kv <= 0.08).all() and (kp >= 0).all() and (kp <= 0.01).all()
        assert (kw >= 0.02).all() and (kw <= 0.1).all() and 0.1 == 2 * 0.05
        assert (mass >= 0.85 * workload.MASS12).all() and (mass <= 1.15 * workload.MASS12).all()
        assert (inertia >= 0.8).all() and (inertia <= 1.25).all() and 0.8 * 1.25 == 1.0
    assert workload.MASS12 == srb12.default_params(10).mass == oracle.params12(10).mass
    assert not np.array_equal(workload.plant_tables12(16, 5)[0], workload.plant_tables12(16, 6)[0])
    assert not np.array_equal(workload.plant_tables12(16, 5)[0], workload.plant_tables(16, 5)[0])
    # replicate_scenes on a make_scenes12 dict: every array tiled scene-major
    sc = workload.make_scenes12(2, 4, 10, "trot", seed=5, n_obs=5)
    rep = workload.replicate_scenes(sc, 3)
    assert set(rep) == set(sc)
    for k, v in sc.items():
        assert rep[k].shape == (3 * v.shape[0],) + v.shape[1:] and rep[k].dtype == v.dtype, k
        for i in range(3):
            assert np.array_equal(rep[k][i * v.shape[0]:(i + 1) * v.shape[0]], v), (k, i)
    after = others()
    assert len(before) == len(after) > 15
    for v, w in zip(before, after):
        assert np.array_equal(v, w)
