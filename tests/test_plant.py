"""The disturbed plant of the LIP rollout (srb_plant), the part that needs no GPU: the numpy Philox of
plant_oracle.py against Random123's known answers, the exact word -> (-1, 1) conversion, the struct's layout, the
refusals by name, the ABI version, and the workload helpers.  The GPU half is test_plant_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import oracle
import plant_oracle
import srbnmpc
from srbnmpc import workload

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
NEW_SYMBOLS = ("srb_sim_advance_plant_device", "srb_rollout_plant_device")
FIELDS = ("struct_size", "seed", "kick_v", "kick_p", "plant_hcom", "n_push", "push_cycle", "push_agent", "push_dv",
          "dist_log")


# ---- Random123 kat_vectors, philox4x32 10: counter, key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_reproduces_the_random123_known_answers():
    for ctr, key, want in KAT:
        got = plant_oracle.philox4x32_10(np.array(ctr), np.array(key))
        assert got.dtype == np.uint32 and [int(v) for v in got] == list(want), (ctr, [hex(int(v)) for v in got])
    # vectorised over rows, each row the scalar answer
    ctrs, keys = np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT])
    assert np.array_equal(plant_oracle.philox4x32_10(ctrs, keys), np.array([k[2] for k in KAT], dtype=np.uint32))


def test_the_uniform_conversion_is_exact_and_inside_the_open_interval():
    from fractions import Fraction
    words = np.array([0, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32)
    u = plant_oracle.uniform(words)
    signed = [0, 2 ** 31 - 1, -2 ** 31, -1]
    for w, s, v in zip(words, signed, u):
        assert Fraction(float(v)) == (Fraction(s) + Fraction(1, 2)) / 2 ** 31, hex(int(w))     # no rounding anywhere
        assert -1.0 < v < 1.0 and v != 0.0
    assert u[1] == 1.0 - 2.0 ** -32 and u[2] == -1.0 + 2.0 ** -32 and u[0] == 2.0 ** -32 and u[3] == -2.0 ** -32
    # kicks(): the seed's halves are the key, (cycle, row) the counter
    seed = (0x299f31d0 << 32) | 0xa4093822
    got = plant_oracle.kicks(seed, 0x243f6a88, [0x85a308d3])
    w = plant_oracle.philox4x32_10(np.array([0x243f6a88, 0x85a308d3, 0, 0]), np.array([0xa4093822, 0x299f31d0]))
    assert np.array_equal(got[0], plant_oracle.uniform(w))


def test_the_restated_discretisation_is_the_models_at_the_models_height():
    p = oracle.params(10, 2)
    Ad, Bd = plant_oracle.lip(p.grav, np.array([p.hcom, 0.25]), p.Ts)
    w2, T = p.grav / p.hcom, p.Ts
    # the series by hand for the entries of one 2 x 2 block (the other block is the same)
    assert Ad[0, 0, 0] == 1.0 + 0.5 * w2 * T * T and Ad[0, 0, 1] == T + w2 * T * T * T / 6
    assert Ad[0, 1, 0] == w2 * T + (w2 * w2) * T * T * T / 6 and Ad[0, 1, 1] == Ad[0, 0, 0]
    assert np.array_equal(Ad[0, :2, :2], Ad[0, 2:, 2:]) and not Ad[0, :2, 2:].any() and not Ad[0, 2:, :2].any()
    assert not np.array_equal(Ad[0], Ad[1])
    # the oracle's own orc_lip builds the QP's equality rows: the solved X follows this Ad, Bd (checked on the GPU)
    assert abs(Bd[0, 0, 0] - (1.0 - Ad[0, 0, 0])) < 1e-15 and Bd[0, 0, 1] == 0.0


def test_plant_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbnmpc.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(FIELDS) + '\\n", sizeof(srb_plant)'
                   + "".join(f", offsetof(srb_plant, {n})" for n in FIELDS) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = srbnmpc.Plant
    assert [f[0] for f in S._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in FIELDS]
    assert S().struct_size == ctypes.sizeof(S)


def test_abi_version_is_still_6_and_the_new_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    assert "#define SRB_ABI_VERSION 6\n" in hdr and "typedef struct srb_plant {" in hdr
    assert srbnmpc.lib().srb_abi_version() == 6 and srbnmpc.ABI_VERSION == 6
    assert srbnmpc.Batch._fields_[-1][0] == "plan" and srbnmpc.Sim._fields_[-1][0] == "distance_to_fail"
    assert [f[0] for f in srbnmpc.AgentSizes._fields_][-1] == "collide_cycle"
    for name in NEW_SYMBOLS:
        assert hasattr(srbnmpc.lib(), name), name


def refusal_cases():
    """(keep-alive arrays, [(plant, word, needs sim.x missing)]) of every refusal of srb_plant.  None needs a
    context: a null context reaches them (test_plant_gpu.py repeats them on a live one)."""
    tab, ci, dv = np.ones(3), np.zeros(3, np.int32), np.zeros((3, 2))
    pt, pi, pv = tab.ctypes.data_as(_dp), ci.ctypes.data_as(_ip), dv.ctypes.data_as(_dp)
    P = srbnmpc.Plant
    bad_size = P()
    bad_size.struct_size += 8
    cases = [(bad_size, "srb_plant.struct_size", False),
             (P(0, pt, None, None, -1, pi, pi, pv, None), "srb_plant.n_push: 0 .. 4096", False),
             (P(0, pt, None, None, 4097, pi, pi, pv, None), "srb_plant.n_push: 0 .. 4096", False),
             (P(0, None, None, None, 3, None, pi, pv, None), "srb_plant.n_push > 0 needs push_cycle", False),
             (P(0, None, None, None, 3, pi, None, pv, None), "srb_plant.n_push > 0 needs push_cycle", False),
             (P(0, None, None, None, 3, pi, pi, None, None), "srb_plant.n_push > 0 needs push_cycle", False),
             (P(7, None, None, pt, 0, None, None, None, None), "srb_plant.plant_hcom needs srb_sim.x", True)]
    return (tab, ci, dv), cases


def call_refused(lib, h, entry, plant, sim, b=None, n_agents=1):
    b = srbnmpc.Batch() if b is None else b
    if entry == "rollout":
        return lib.srb_rollout_plant_device(h, n_agents, ctypes.byref(b), ctypes.byref(sim), None, None, None,
                                            ctypes.byref(plant), 1, None)
    return lib.srb_sim_advance_plant_device(h, n_agents, ctypes.byref(sim), ctypes.byref(plant), sim.c_first, None)


def test_refusals_by_name_without_a_context():
    lib = srbnmpc.lib()
    keep, cases = refusal_cases()
    goal = np.zeros(2)
    for entry in ("advance", "rollout"):
        for plant, word, sim_x in cases:
            if sim_x and entry == "rollout":
                continue                                          # the rollout reads batch.x and names that itself
            sim = srbnmpc.Sim()
            sim.goal = goal.ctypes.data_as(_dp)
            assert call_refused(lib, None, entry, plant, sim) == -1, (entry, word)
            assert word in lib.srb_last_error().decode(), (entry, word, lib.srb_last_error())
    # a struct that passes gets as far as the missing context, with the plant on or with nothing set
    sim = srbnmpc.Sim()
    sim.goal = goal.ctypes.data_as(_dp)
    for plant in (srbnmpc.Plant(1, keep[0].ctypes.data_as(_dp), None, None, 0, None, None, None, None), srbnmpc.Plant()):
        for entry in ("advance", "rollout"):
            assert call_refused(lib, None, entry, plant, sim) == -1
            assert "null argument" in lib.srb_last_error().decode(), (entry, lib.srb_last_error())
    # the struct-size refusal of srb_sim comes first, as in every srb_sim entry point
    bad = srbnmpc.Sim()
    bad.struct_size -= 8
    assert call_refused(lib, None, "advance", cases[1][0], bad) == -1
    assert "srb_sim.struct_size" in lib.srb_last_error().decode()


def test_plant_tables_and_replicas_are_deterministic_and_leave_the_other_draws_alone():
    def others():
        """every other draw of the module, as a flat list of arrays"""
        out = []
        for v in (workload.make_batch(8, 10, 2, seed=5), workload.make_scenes(2, 4, 10, 2, seed=5, n_obs=5),
                  workload.agent_sizes(16, 5), workload.obstacle_sizes(20, 5), workload.obstacle_velocities(20, 5)):
            vals = list(v.values()) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else [v]
            out += [np.array(x) for x in vals if isinstance(x, np.ndarray)]
        return out
    before = others()
    for n, seed in ((16, 5), (320, 12), (1, 0)):
        kv, kp, hc = workload.plant_tables(n, seed)
        for v, w in zip((kv, kp, hc), workload.plant_tables(n, seed)):
            assert v.shape == (n,) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] and np.array_equal(v, w)
        g = np.random.default_rng(400 + seed)
        assert np.array_equal(kv, g.uniform(0.02, 0.08, n)) and np.array_equal(kp, g.uniform(0.0, 0.01, n))
        assert np.array_equal(hc, workload.HCOM * g.uniform(0.85, 1.15, n))
        # the ranges the docstring states: a fraction of VREF, at most one grid step at VREF, 15 % of the height
        assert (kv >= 0.02).all() and (kv <= 0.08).all() and 0.08 < 0.3 * workload.VREF
        assert (kp >= 0).all() and (kp <= 0.01).all() and 0.01 < workload.VREF * workload.TS
        assert (hc >= 0.85 * workload.HCOM).all() and (hc <= 1.15 * workload.HCOM).all()
    assert workload.HCOM == srbnmpc.default_params(10, 2).hcom
    assert not np.array_equal(workload.plant_tables(16, 5)[0], workload.plant_tables(16, 6)[0])
    sc = workload.make_scenes(2, 4, 10, 2, seed=5, n_obs=5)
    rep = workload.replicate_scenes(sc, 3)
    assert set(rep) == set(sc)
    for k, v in sc.items():
        assert rep[k].shape == (3 * v.shape[0],) + v.shape[1:] and rep[k].dtype == v.dtype, k
        for i in range(3):
            assert np.array_equal(rep[k][i * v.shape[0]:(i + 1) * v.shape[0]], v), (k, i)
    one = workload.replicate_scenes(sc, 1)
    assert all(np.array_equal(one[k], sc[k]) for k in sc)
    with pytest.raises(ValueError, match="copies"):
        workload.replicate_scenes(sc, 0)
    after = others()
    assert len(before) == len(after) > 10
    for v, w in zip(before, after):
        assert np.array_equal(v, w)


def test_rollout12_refuses_the_plant_arguments_by_name():
    import inspect
    from srbnmpc import srb12
    sig = inspect.signature(srb12.Rollout12.__init__).parameters
    for name, val in (("plant_seed", 3), ("kick_v", np.zeros(2)), ("kick_p", np.zeros(2)), ("plant_hcom", np.ones(2)),
                      ("pushes", (None, None, None))):
        assert name in sig
        with pytest.raises(ValueError, match=f"Rollout12: {name} is not available"):
            srb12.Rollout12(None, None, **{name: val})
