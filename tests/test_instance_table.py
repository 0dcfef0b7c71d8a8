"""CPU tests of the kernel-instance tables and the host's picks (srb_kernel_table / srb_pick_kernel and the SRB-12
pair; no device): every shipped instance can be picked by some admissible shape, no pick returns an instance the shape
does not fit, and a shape with a compiled instance at the wanted wave count gets it.  No list of unreachable entries
is kept here: an entry nothing picks is four to six kernels compiled for nothing, and fails the test.

Admissible shapes: N 2..33, C 2..4, K_obs + K_nbr 0..32 (K_obs = min(K, 16), the rest K_nbr), waves 1, 2, 4, where
srb_check_params accepts them; SRB-12: N 1..24, K 0..32 where srb12_check_params accepts them.
"""
import ctypes

import srbnmpc
from srbnmpc import srb12


def slots(N, C, K):
    """Row slots of one agent (csrc/srb_kernel_params.h srb_slots)."""
    return (6 + C) * N + 1 + 2 * (N - 1) + 2 * N + N * K


def lip_params(N, C, K):
    return srbnmpc.default_params(N, C, K_obs=min(K, 16), K_nbr=max(K - 16, 0))


def lip_shapes():
    for N in range(1, 34):
        for C in (2, 3, 4):
            for K in range(0, 33):
                if srbnmpc.check_params(lip_params(N, C, K)):
                    yield N, C, K


_picks = {}


def lip_picks():
    """{(N, C, K, waves): dims} over every admissible shape, computed once."""
    if not _picks:
        for N, C, K in lip_shapes():
            for w in (1, 2, 4):
                _picks[(N, C, K, w)] = srbnmpc.pick_kernel(lip_params(N, C, K), w)
    return _picks


def test_table_lists_the_fp64_instances_then_the_fp32_ones():
    tab = srbnmpc.kernel_table()
    names = [n for _, n in tab]
    assert len(set(names)) == len(names)
    f32 = ["_f32_" in n for n in names]
    assert any(f32) and not all(f32) and f32 == sorted(f32)               # the f32 entries follow the fp64 ones
    for d, n in tab:
        assert n == ("srb_nmpc_kernel_f32_" if "_f32_" in n else "srb_nmpc_kernel_") + "_".join(map(str, d))
        assert all((d[3] > 0) == (x > 0) for x in d[3:])                  # a shape is compiled whole or not at all
    f64 = {d for d, n in tab if "_f32_" not in n}
    assert all(d in f64 for d, n in tab if "_f32_" in n)                  # an f32 entry is a variant of an fp64 one
    lib, d6, nm = srbnmpc.lib(), (ctypes.c_int * 6)(), ctypes.c_char_p()
    assert lib.srb_kernel_table(len(tab), d6, ctypes.byref(nm)) == -1     # SRB_ERR_ARG past the end
    assert lib.srb_kernel_table(-1, d6, ctypes.byref(nm)) == -1


def test_the_admissible_shapes_are_what_the_header_promises():
    sh = set(lip_shapes())
    assert len(sh) > 1000
    for N, C, K in sh:
        assert 2 <= N <= 33 and N * (C - 1) + 1 <= 32
    assert (10, 2, 11) in sh and (20, 2, 11) in sh and (4, 4, 1) in sh and (31, 2, 0) in sh
    assert (1, 2, 0) not in sh and (32, 2, 0) not in sh and (11, 4, 0) not in sh


def test_every_lip_instance_is_picked_by_some_shape():
    picked = set(lip_picks().values())
    f64 = [d for d, n in srbnmpc.kernel_table() if "_f32_" not in n]
    missing = [d for d in f64 if d not in picked]
    assert not missing, f"no admissible shape picks {missing}"
    assert picked <= set(f64)


def test_a_lip_pick_fits_its_shape():
    for (N, C, K, w), (nzl, ts, nw, nc, cc, kc) in lip_picks().items():
        key = (N, C, K, w, (nzl, ts, nw, nc, cc, kc))
        assert N * (C - 1) + 1 <= nzl, key
        assert slots(N, C, K) <= 64 * nw * ts, key
        assert (nc, cc, kc) in ((0, 0, 0), (N, C, K)), key
        assert nw <= w, key                                   # never more waves than wanted


def test_a_shape_with_a_compiled_instance_gets_it():
    tab = [d for d, n in srbnmpc.kernel_table() if "_f32_" not in n]
    compiled = [d for d in tab if d[3] > 0]
    assert compiled
    for d in compiled:
        nzl, ts, nw, N, C, K = d
        assert N * (C - 1) + 1 <= nzl and slots(N, C, K) <= 64 * nw * ts, d    # the entry fits its own shape
        assert lip_picks()[(N, C, K, nw)] == d
    # and nothing else gets a compiled entry
    for (N, C, K, w), d in lip_picks().items():
        if d[3] > 0:
            assert d[3:] == (N, C, K) and d[2] == w


def test_no_pick_is_dominated():
    """The pick is never an entry that another run-time entry of the same wave count undercuts in both bounds (NZL and
    TS, one of them strictly) while fitting the shape too: such an order would make the smaller entry dead code and
    cost the shape its fused polish (NZL <= 24) or its stored obstacle rows (NZL <= 16)."""
    run_time = [d for d, n in srbnmpc.kernel_table() if "_f32_" not in n and d[3] == 0]
    for (N, C, K, w), d in lip_picks().items():
        if d[3] > 0:
            continue
        better = [e for e in run_time if e[2] == d[2] and e != d and e[0] <= d[0] and e[1] <= d[1] and
                  e[0] >= N * (C - 1) + 1 and 64 * e[2] * e[1] >= slots(N, C, K)]
        assert not better, (N, C, K, w, d, better)


def test_pick_kernel_refuses_what_it_cannot_serve():
    lib, d6 = srbnmpc.lib(), (ctypes.c_int * 6)()
    p = lip_params(10, 2, 3)
    assert lib.srb_pick_kernel(ctypes.byref(p), 3, d6) == -1
    assert lib.srb_pick_kernel(None, 1, d6) == -1
    assert lib.srb_pick_kernel(ctypes.byref(lip_params(31, 2, 32)), 1, d6) == -3   # SRB_ERR_SIZE: 1363 slots


# ---------------------------------------------------------------------------- SRB-12
def shapes12():
    for N in range(1, 25):
        for K in range(0, 33):
            if srb12.check_params(srb12.default_params(N, K_obs=min(K, 16), K_nbr=max(K - 16, 0))):
                yield N, K


def test_table12_names():
    tab = srb12.kernel_table()
    assert len(set(d for d, _ in tab)) == len(tab) >= 4
    for d, n in tab:
        assert n == "srb12_kernel_" + "_".join(map(str, d))
        assert (d[2] > 0) == (d[3] > 0)
    d4, nm = (ctypes.c_int * 4)(), ctypes.c_char_p()
    assert srbnmpc.lib().srb12_kernel_table(len(tab), d4, ctypes.byref(nm)) == -1


def test_every_srb12_instance_is_picked_and_every_pick_fits():
    sh = list(shapes12())
    assert len(sh) > 500 and (10, 11) in sh and (20, 11) in sh and (6, 0) in sh and (24, 32) in sh
    tab = [d for d, _ in srb12.kernel_table()]
    picked = set()
    for N, K in sh:
        tl, to, nc, k1 = d = srb12.pick_kernel(N, K)
        picked.add(d)
        assert 4 * N <= 64 * tl and N * K <= 64 * to, (N, K, d)
        assert (nc, k1) in ((0, 0), (N, K + 1)), (N, K, d)
        exact = [e for e in tab if (e[2], e[3]) == (N, K + 1)]
        if exact:
            assert d == exact[0], (N, K, d)
        else:                                                  # the cheapest run-time entry that fits: fewest trips
            fit = [e for e in tab if e[2] == 0 and 4 * N <= 64 * e[0] and N * K <= 64 * e[1]]
            assert (tl, to) == min((e[0], e[1]) for e in fit), (N, K, d)
    missing = [d for d in tab if d not in picked]
    assert not missing, f"no admissible shape picks {missing}"
    assert picked <= set(tab)
    d4 = (ctypes.c_int * 4)()
    assert srbnmpc.lib().srb12_pick_kernel(0, 0, d4) == -1
