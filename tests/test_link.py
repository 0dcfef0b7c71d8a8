"""The degraded neighbour link of the LIP rollout (srb_link), the part that needs no GPU: the numpy restatement
(link_oracle.py) against an independent event-list simulation written per row in plain Python, its closed forms, the
struct's layout, the refusals by name and the workload helper.  The GPU half is test_link_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import link_oracle
import plant_oracle
import srbnmpc
from srbnmpc import workload

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
NEW_SYMBOLS = ("srb_link_update_device", "srb_link_update_lanes_device", "srb_rollout_link_device")
FIELDS = ("struct_size", "seed", "delay", "drop", "noise_p", "noise_v", "max_delay", "extrapolate", "ring_state",
          "ring_plan", "held_state", "held_plan", "held_cycle", "seen_state", "seen_plan", "age_log")
TS = workload.TS


# ---------------------------------------------------------------- the independent simulation: messages in flight
def event_sim(c_first, truth_states, truth_plans, tab, N):
    """Per row and in plain Python floats: every message sent after c_first that is not lost goes into a dict keyed by
    the cycle it is delivered at (send cycle + the row's delay); a cycle pops its delivery, if any, and that becomes
    the held message.  Returns (seen_state [T][n][4], seen_plan [T][n][N][2] with NaN where none is written, age [T][n])."""
    T, n = len(truth_states), len(truth_states[0])
    seed, D, Ts, ext = tab["seed"], tab["max_delay"], tab["Ts"], tab["extrapolate"]
    seen = np.full((T, n, 4), np.nan)
    seen_plan = np.full((T, n, N, 2), np.nan)
    ages = np.zeros((T, n), np.int32)
    for g in range(n):
        d = 0 if tab["delay"] is None else min(max(int(tab["delay"][g]), 0), D)
        in_flight, held = {}, None
        for i in range(T):
            c = c_first + i
            msg = [float(v) for v in truth_states[i][g]]
            if tab["noise_p"] is not None or tab["noise_v"] is not None:
                u = [float(v) for v in link_oracle.draws(seed, c, [g], 3)[0]]
                if tab["noise_p"] is not None:
                    b = float(tab["noise_p"][g])
                    msg[0] = msg[0] + b * u[0]
                    msg[1] = msg[1] + b * u[1]
                if tab["noise_v"] is not None:
                    b = float(tab["noise_v"][g])
                    msg[2] = msg[2] + b * u[2]
                    msg[3] = msg[3] + b * u[3]
            plan = None
            if truth_plans is not None and c > c_first:
                plan = [[float(v) for v in q] for q in truth_plans[i][g]]
            if c == c_first:
                held = (c, msg, None)                          # the complete exchange the team starts from
            else:
                lost = False
                if tab["drop"] is not None:
                    u0 = float(link_oracle.draws(seed, c, [g], 2)[0, 0])
                    lost = 0.5 * u0 + 0.5 < float(tab["drop"][g])
                if not lost:
                    in_flight[c + d] = (c, msg, plan)
                if c in in_flight:
                    held = in_flight.pop(c)
            sent, hs, hp = held
            age = c - sent
            ages[i, g] = age
            m = 4 * age if ext else 0
            e = list(hs)
            if m > 0:
                e[0] = hs[0] + hs[2] * (float(m) * Ts)
                e[1] = hs[1] + hs[3] * (float(m) * Ts)
            seen[i, g] = e
            if truth_plans is None or c == c_first:
                continue
            for k in range(N):
                if hp is None:                                 # no plan held yet
                    q = [e[0] + e[2] * (Ts * float(k + 1)), e[1] + e[3] * (Ts * float(k + 1))]
                elif k + m < N:
                    q = hp[k + m]
                else:
                    j = float(k + m - N + 1)
                    q = [hp[N - 1][0] + j * (hp[N - 1][0] - hp[N - 2][0]), hp[N - 1][1] + j * (hp[N - 1][1] - hp[N - 2][1])]
                seen_plan[i, g, k] = q
    return seen, seen_plan, ages


def truth(rng, T, n, N):
    st = np.stack([rng.uniform(0, 9, (T, n)), rng.uniform(-2, 2, (T, n)), rng.uniform(-.3, .3, (T, n)),
                   rng.uniform(-.3, .3, (T, n))], -1)
    return st, rng.uniform(-3, 12, (T, n, N, 2))


def case_tables(rng, n, max_delay, extrapolate, seed=0x0123456789abcdef):
    """Every table; rows 0 / 1 at drop exactly 0 / 1, row 2 and 3 at delay 0 and max_delay (later than the first cycles
    elapsed), one entry above max_delay and one below 0 (clamped)."""
    delay = rng.integers(0, max_delay + 1, n).astype(np.int32)
    delay[2], delay[3], delay[4], delay[5] = 0, max_delay, max_delay + 5, -2
    drop = rng.uniform(0.0, 0.6, n)
    drop[0], drop[1] = 0.0, 1.0
    return link_oracle.tables(seed, delay, drop, rng.uniform(0, 0.03, n), rng.uniform(0, 0.05, n), max_delay, extrapolate)


@pytest.mark.parametrize("N,extrapolate,plans", [(10, 0, True), (10, 1, True), (4, 0, True), (4, 1, True), (4, 1, False)])
def test_the_restatement_agrees_with_an_event_list_simulation(N, extrapolate, plans):
    """12 cycles from c_first = 3 with max_delay 3: seen tables and ages of the ring-buffer restatement equal those of
    the messages-in-flight simulation, bitwise.  With N = 4 the shifted plan is beyond the horizon already at age 1."""
    rng = np.random.default_rng(77 + N + extrapolate)
    T, n, c_first = 12, 9, 3
    st, pl = truth(rng, T, n, N)
    tab = case_tables(rng, n, 3, extrapolate)
    got = link_oracle.run(c_first, st, pl if plans else None, tab, N)
    seen, seen_plan, ages = event_sim(c_first, st, pl if plans else None, tab, N)
    for i, (ss, sp, age, _) in enumerate(got):
        np.testing.assert_array_equal(ss, seen[i], err_msg=f"cycle {i}")
        np.testing.assert_array_equal(age, ages[i], err_msg=f"cycle {i}")
        if plans and i > 0:
            np.testing.assert_array_equal(sp, seen_plan[i], err_msg=f"cycle {i}")
        else:
            assert sp is None
    assert (ages[:, 0] == np.minimum(tab["delay"][0], np.arange(T))).all()            # drop 0
    assert (ages[:, 1] == np.arange(T)).all()                                          # drop 1
    assert ages.max() > 3                                                              # losses age a row past its delay
    if extrapolate:
        assert (seen[5, 1, :2] != got[0][0][1, :2]).all() and (seen[5, 1, 2:] == got[0][0][1, 2:]).all()
    else:
        np.testing.assert_array_equal(seen[5, 1], got[0][0][1])                        # held as it is


def test_closed_forms_of_the_age():
    rng = np.random.default_rng(5)
    T, n, N, c_first = 9, 6, 4, 2
    st, pl = truth(rng, T, n, N)
    delay = np.array([0, 1, 2, 3, 3, 1], np.int32)
    for tab, want in ((link_oracle.tables(3, delay), lambda i: np.minimum(delay, i)),
                      (link_oracle.tables(3, delay, np.zeros(n)), lambda i: np.minimum(delay, i)),
                      (link_oracle.tables(3, delay, np.ones(n)), lambda i: np.full(n, i))):
        for i, (ss, sp, age, _) in enumerate(link_oracle.run(c_first, st, pl, tab, N)):
            np.testing.assert_array_equal(age, want(i))
            if tab["drop"] is None:                          # no noise: what is seen is the truth of `age` cycles ago
                np.testing.assert_array_equal(ss, st[i - age, np.arange(n)])
    # delay 0, no loss, no noise: the perceived tables are the truth, with either extrapolate setting
    for ext in (0, 1):
        for i, (ss, sp, age, _) in enumerate(link_oracle.run(c_first, st, pl, link_oracle.tables(3, np.zeros(n, np.int32), extrapolate=ext), N)):
            np.testing.assert_array_equal(ss, st[i])
            assert (age == 0).all() and (sp is None if i == 0 else np.array_equal(sp, pl[i]))


def test_the_plan_shift_is_shift4_at_age_one_and_the_draws_are_their_own():
    rng = np.random.default_rng(9)
    for N in (4, 10):
        x = rng.normal(size=(5, 6 * N + 1))
        P = x[:, :4 * N].reshape(5, N, 4)[:, :, [0, 2]]
        import sim_oracle
        np.testing.assert_array_equal(link_oracle.shift(P, np.full(5, 4)), sim_oracle.shift4(N, x))
        np.testing.assert_array_equal(link_oracle.shift(P, np.zeros(5, np.int64)), P)
    seed, rows = 0x5eed5eed12345678, np.arange(7)
    k = plant_oracle.kicks(seed, 11, rows)
    loss, noise = link_oracle.draws(seed, 11, rows, 2), link_oracle.draws(seed, 11, rows, 3)
    assert (loss != k).all() and (noise != k).all() and (loss != noise).all()
    w = plant_oracle.philox4x32_10(np.array([11, 4, 3, 0]), np.array([seed & 0xffffffff, seed >> 32]))
    np.testing.assert_array_equal(noise[4], plant_oracle.uniform(w))
    u0 = link_oracle.draws(seed, np.arange(2000), np.zeros(2000, np.int64), 2)[:, 0]
    assert (0.5 * u0 + 0.5 > 0).all() and (0.5 * u0 + 0.5 < 1).all()                   # 0 never loses, 1 always


def test_link_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(FIELDS) + '\\n", sizeof(srb_link)'
                   + "".join(f", offsetof(srb_link, {n})" for n in FIELDS) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = srbnmpc.Link
    assert [f[0] for f in S._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in FIELDS]
    assert S().struct_size == ctypes.sizeof(S)
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr and srbnmpc.lib().srb_abi_version() == 6
    assert srbnmpc.Plant._fields_[-1][0] == "dist_log" and srbnmpc.Sim._fields_[-1][0] == "distance_to_fail"
    for name in NEW_SYMBOLS:
        assert hasattr(srbnmpc.lib(), name), name


def make_link(keep, **kw):
    """A srbnmpc.Link on host arrays (never dereferenced: every call here is refused first); keep holds them alive."""
    n = 3
    f = lambda *sh: keep.setdefault(len(keep), np.zeros(sh))
    i = lambda *sh: keep.setdefault(len(keep), np.zeros(sh, np.int32))
    d = dict(seed=1, delay=i(n).ctypes.data_as(_ip), drop=None, noise_p=None, noise_v=None, max_delay=2, extrapolate=0,
             ring_state=f(3, n, 4).ctypes.data_as(_dp), ring_plan=f(3, n, 4, 2).ctypes.data_as(_dp),
             held_state=f(n, 4).ctypes.data_as(_dp), held_plan=f(n, 4, 2).ctypes.data_as(_dp),
             held_cycle=i(n).ctypes.data_as(_ip), seen_state=f(n, 4).ctypes.data_as(_dp),
             seen_plan=f(n, 4, 2).ctypes.data_as(_dp), age_log=None)
    d.update(kw)
    return srbnmpc.Link(*[d[k] for k in FIELDS[1:]])


def refusal_cases(keep):
    """[(link, word, needs a plan table)] of every refusal of srb_link that needs no context."""
    bad_size = make_link(keep)
    bad_size.struct_size += 8
    cases = [(bad_size, "srb_link.struct_size", False),
             (make_link(keep, max_delay=-1), "srb_link.max_delay: 0 .. 16", False),
             (make_link(keep, max_delay=17), "srb_link.max_delay: 0 .. 16", False),
             (make_link(keep, delay=None, max_delay=17), "srb_link.max_delay: 0 .. 16", False),    # even when off
             (make_link(keep, extrapolate=2), "srb_link.extrapolate: 0", False),
             (make_link(keep, extrapolate=-1), "srb_link.extrapolate: 0", False)]
    for name in ("ring_state", "held_state", "held_cycle", "seen_state"):
        cases.append((make_link(keep, **{name: None}), "a link that is on needs ring_state", False))
    for name in ("ring_plan", "held_plan", "seen_plan"):
        cases.append((make_link(keep, **{name: None}), "a plan table needs ring_plan", True))
    return cases


def test_refusals_by_name_without_a_context():
    lib = srbnmpc.lib()
    keep = {}
    err = lambda: lib.srb_last_error().decode()
    last, plan, goal = np.zeros((3, 4)), np.zeros((3, 4, 2)), np.zeros(2)
    lp, pp = last.ctypes.data_as(_dp), plan.ctypes.data_as(_dp)
    for link, word, needs_plan in refusal_cases(keep):
        assert lib.srb_link_update_device(None, 3, ctypes.byref(link), lp, pp, 1, 0, None) == -1 and word in err(), (word, err())
        if needs_plan:                                         # without a plan table the plan buffers may be absent
            assert lib.srb_link_update_device(None, 3, ctypes.byref(link), lp, None, 1, 0, None) == -1
            assert "null argument" in err(), err()
        sim = srbnmpc.Sim()
        sim.goal, sim.last_state, sim.plan_table = goal.ctypes.data_as(_dp), lp, pp
        rc = lib.srb_rollout_link_device(None, 3, ctypes.byref(srbnmpc.Batch()), ctypes.byref(sim), None, None, None, None,
                                         ctypes.byref(link), 1, None)
        assert rc == -1 and word in err(), (word, err())
    # seen_state overlapping last_state (here: its second row onwards)
    over = make_link(keep, seen_state=ctypes.cast(ctypes.c_void_p(last.ctypes.data + 32), _dp))
    assert lib.srb_link_update_device(None, 3, ctypes.byref(over), lp, None, 1, 0, None) == -1
    assert "srb_link.seen_state overlaps last_state" in err()
    assert lib.srb_link_update_lanes_device(None, 3, ctypes.byref(make_link(keep)), lp, None, 1, 0, 4, None) == -1
    assert "lanes is 1, 8 or 16" in err()
    assert lib.srb_link_update_device(None, 3, ctypes.byref(make_link(keep)), lp, None, 1, 2, None) == -1
    assert "cycle precedes c_first" in err()
    # a struct that passes gets as far as the missing context, on or off, and so does no link at all
    for link in (make_link(keep), make_link(keep, delay=None), srbnmpc.Link()):
        assert lib.srb_link_update_device(None, 3, ctypes.byref(link), lp, pp, 1, 0, None) == -1
        assert "null argument" in err(), err()
    sim = srbnmpc.Sim()
    sim.goal = goal.ctypes.data_as(_dp)
    assert lib.srb_rollout_link_device(None, 3, ctypes.byref(srbnmpc.Batch()), ctypes.byref(sim), None, None, None, None,
                                       None, 1, None) == -1 and "null argument" in err()
    # the struct-size refusal of srb_sim comes first, as in every srb_sim entry point
    bad = srbnmpc.Sim()
    bad.struct_size -= 8
    assert lib.srb_rollout_link_device(None, 3, ctypes.byref(srbnmpc.Batch()), ctypes.byref(bad), None, None, None, None,
                                       ctypes.byref(make_link(keep, max_delay=17)), 1, None) == -1
    assert "srb_sim.struct_size" in err()


def test_link_tables_are_deterministic_documented_and_leave_the_other_draws_alone():
    before = [workload.plant_tables(16, 5), workload.agent_sizes(16, 5), workload.make_batch(8, 10, 2, seed=5)["x0"]]
    for n, seed in ((16, 5), (320, 12), (1, 0)):
        tabs = workload.link_tables(n, seed)
        for v, w, dt in zip(tabs, workload.link_tables(n, seed), (np.int32, np.float64, np.float64, np.float64)):
            assert v.shape == (n,) and v.dtype == dt and v.flags["C_CONTIGUOUS"] and np.array_equal(v, w)
        delay, drop, noise_p, noise_v = tabs
        g = np.random.default_rng(600 + seed)
        assert np.array_equal(delay, g.integers(0, 3, n)) and np.array_equal(drop, g.uniform(0, 0.3, n))
        assert np.array_equal(noise_p, g.uniform(0, 0.03, n)) and np.array_equal(noise_v, g.uniform(0, 0.03, n))
        # the ranges the docstring states, in terms of the cycle time 4 Ts and VREF
        assert delay.min() >= 0 and delay.max() <= 2 and abs(4 * TS - 0.172) < 1e-12
        assert (drop >= 0).all() and (drop <= 0.3).all()
        assert (noise_p >= 0).all() and (noise_p <= 0.03).all() and 0.03 < workload.VREF * 4 * TS
        assert (noise_v >= 0).all() and (noise_v <= 0.03).all() and 0.03 < 0.12 * workload.VREF
    assert not np.array_equal(workload.link_tables(64, 5)[1], workload.link_tables(64, 6)[1])
    after = [workload.plant_tables(16, 5), workload.agent_sizes(16, 5), workload.make_batch(8, 10, 2, seed=5)["x0"]]
    flat = lambda vs: [np.asarray(x) for v in vs for x in (v if isinstance(v, tuple) else [v])]
    assert all(np.array_equal(a, b) for a, b in zip(flat(before), flat(after)))
    m = srbnmpc.LinkModel()
    assert not m.on and srbnmpc.LinkModel(delay=delay).on and srbnmpc.LinkModel(noise_v=noise_v).on
