"""GPU tests of the scene partition (srb_ctx_set_scenes; csrc/srb_scenes.hip, srbnmpc.BatchSolver.set_scenes,
srbnmpc.Rollout.scene_results): a batch of independent teams selected, solved, advanced and measured by the same
launches must give, bit for bit, what every team gives alone through the unsegmented entry points.  Every
comparison is exact (np.array_equal); both sides run with set_waves(1), since the automatic wave count depends
on the batch size and changes the summation order."""
import ctypes
import re

import numpy as np
import pytest

import srbnmpc
from srbnmpc import workload

gpu = pytest.mark.gpu
N, C = 10, 2


def _need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if v is not None}


def new_solver(Ko, Kn, max_agents, scenes=None, plan_selection=False, n=N, c=C):
    s = srbnmpc.BatchSolver(srbnmpc.default_params(n, c, K_obs=Ko, K_nbr=Kn), max_agents)
    s.set_waves(1)
    if scenes:
        s.set_scenes(*scenes)
        assert s.scenes == tuple(scenes)
    if plan_selection:
        s.set_option("plan_selection", 1)
    return s


def scene_batch(S, sa, so, seed, duplicates=False):
    """make_scenes without the start clearance (any density), optionally with tied rows: in every scene obstacle 1
    repeats obstacle 0 and, from three agents on, agent 2 stands on agent 1."""
    b = workload.make_scenes(S, sa, N, C, seed=seed, n_obs=so, clearance=0.0)
    if duplicates:
        for s in range(S):
            if so >= 2:
                b["obstacles"][s * so + 1] = b["obstacles"][s * so]
            if sa >= 3:
                b["nbr_state"][s * sa + 2, :2] = b["nbr_state"][s * sa + 1, :2]
    return b


def plans_of(b, seed):
    """A plan table [A][N][2]: the constant-velocity line of every snapshot row, bent by a little noise."""
    rng = np.random.default_rng(seed)
    nb = b["nbr_state"]
    t = workload.TS * np.arange(1, N + 1)
    return np.ascontiguousarray(nb[:, None, :2] + nb[:, None, 2:] * t[None, :, None] + rng.normal(0, 0.05, (nb.shape[0], N, 2)))


def select(torch, s, x0, ob, nb, tables=3, agent_offset=0, nbr_plan=None):
    """sel of one srb_select_device call, on the host; columns the call does not write keep -7."""
    Ko, Kn = s.n_selected(0 if ob is None else ob.shape[0], 0 if nb is None else nb.shape[0])
    sel = torch.full((x0.shape[0], Ko + Kn), -7, dtype=torch.int32, device="cuda")
    s.select_device(dev(torch, x0), dev(torch, ob) if ob is not None and ob.shape[0] else None, dev(torch, nb), sel,
                    tables=tables, agent_offset=agent_offset, nbr_plan=dev(torch, nbr_plan))
    torch.cuda.synchronize()
    return sel.cpu().numpy(), Ko, Kn


def rebase(sel, Ko, ob0, nb0):
    """Scene-local indices of an unsegmented call as global rows: the bases added, -1 and the -7 sentinel kept."""
    out = sel.copy()
    out[:, :Ko] = np.where(sel[:, :Ko] >= 0, sel[:, :Ko] + ob0, sel[:, :Ko])
    out[:, Ko:] = np.where(sel[:, Ko:] >= 0, sel[:, Ko:] + nb0, sel[:, Ko:])
    return out


def per_scene_select(torch, u, b, S, sa, so, tables, plan=None):
    rows = []
    for s in range(S):
        a, o = slice(s * sa, (s + 1) * sa), slice(s * so, (s + 1) * so)
        sel, Ko, Kn = select(torch, u, b["x0"][a], b["obstacles"][o] if so else None, b["nbr_state"][a], tables,
                             nbr_plan=None if plan is None else plan[a])
        rows.append(rebase(sel, Ko, s * so, s * sa))
    return np.concatenate(rows)


# ================================================================================== selection
@gpu
@pytest.mark.parametrize("sa,so,Ko,Kn", [(3, 0, 3, 2), (3, 1, 3, 2), (3, 5, 3, 2), (3, 70, 3, 2), (4, 5, 3, 8), (1, 5, 3, 2)])
def test_selection_equals_per_scene_selection(sa, so, Ko, Kn):
    """One scene-batched srb_select_device call against unsegmented calls on each scene's own tables, indices
    re-based: tables 1, 2, 3 and the horizon-aware selection, with tied rows in every scene.  so = 70 is more than
    one row a lane, (4, K_nbr 8) clamps to 3 neighbour rows and team 1 has none; so = 0 has no static rows."""
    torch = _need_gpu()
    S = 5
    b = scene_batch(S, sa, so, seed=10 * sa + so, duplicates=True)
    plan = plans_of(b, 1)
    ob = b["obstacles"] if so else None
    for plan_sel in (False, True):
        s = new_solver(Ko, Kn, S * sa, scenes=(sa, so), plan_selection=plan_sel)
        u = new_solver(Ko, Kn, S * sa, plan_selection=plan_sel)
        assert s.n_selected(S * so, S * sa) == (min(Ko, so), min(Kn, sa - 1))
        for tables in (1, 2, 3):
            pl = plan if plan_sel else None
            got, ko, kn = select(torch, s, b["x0"], ob, b["nbr_state"], tables, nbr_plan=pl)
            assert (ko, kn) == (min(Ko, so), min(Kn, sa - 1)) and got.shape == (S * sa, ko + kn)
            want = per_scene_select(torch, u, b, S, sa, so, tables, pl)
            assert np.array_equal(got, want), (plan_sel, tables, got[:6].tolist(), want[:6].tolist())
            if tables & 1 and ko:
                sc = np.arange(S * sa) // sa
                assert ((got[:, :ko] >= sc[:, None] * so) & (got[:, :ko] < (sc[:, None] + 1) * so)).all()
            if tables & 2 and kn:
                sc = np.arange(S * sa) // sa
                nbc = got[:, ko:]
                assert ((nbc >= sc[:, None] * sa) & (nbc < (sc[:, None] + 1) * sa)).all()
                assert (nbc != np.arange(S * sa)[:, None]).all()          # the self row is never selected
        s.close(); u.close()


@gpu
def test_selection_without_ties_equals_a_numpy_sort():
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 5, 6, 9, 3, 4
    b = scene_batch(S, sa, so, seed=3)
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    got, ko, kn = select(torch, s, b["x0"], b["obstacles"], b["nbr_state"])
    s.close()
    assert (ko, kn) == (Ko, Kn)
    for g in range(S * sa):
        sc = g // sa
        p = b["x0"][g, [0, 2]]
        do = np.sqrt(((b["obstacles"][sc * so:(sc + 1) * so] - p) ** 2).sum(1))
        dn = np.sqrt(((b["nbr_state"][sc * sa:(sc + 1) * sa, :2] - p) ** 2).sum(1))
        dn[g - sc * sa] = np.inf
        assert len(set(do)) == so and len(set(dn)) == sa                  # no ties: the sort is the order
        assert got[g, :Ko].tolist() == (np.argsort(do)[:Ko] + sc * so).tolist(), g
        assert got[g, Ko:].tolist() == (np.argsort(dn)[:Kn] + sc * sa).tolist(), g


@gpu
def test_rules_restated_per_scene():
    """The static 1000 m rule selects the scene's own row 0; NaN neighbour rows are never selected and the columns
    they leave are -1 (of three others: one NaN row leaves one -1, two NaN rows leave two); the self row is never
    selected."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 3, 4, 5, 3, 3
    b = scene_batch(S, sa, so, seed=4)
    b["obstacles"][so:2 * so] += 5000.0                       # scene 1: every obstacle beyond 1000 m
    b["nbr_state"][2 * sa + 1, 0] = np.nan                    # scene 2: rows 1 and 3 of its four are NaN
    b["nbr_state"][2 * sa + 3, 1] = np.nan
    b["nbr_state"][0 * sa + 2, 0] = np.nan                    # scene 0: row 2 is NaN
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    u = new_solver(Ko, Kn, S * sa)
    got, ko, kn = select(torch, s, b["x0"], b["obstacles"], b["nbr_state"])
    want = per_scene_select(torch, u, b, S, sa, so, 3)
    s.close(); u.close()
    assert np.array_equal(got, want)
    assert (got[sa:2 * sa, :Ko] == 1 * so).all()              # the scene's row 0, not the table's
    assert (got[:sa, :Ko] < so).all() and (got[:sa, :Ko] >= 0).all() and (got[2 * sa:, :Ko] >= 2 * so).all()
    assert got[2 * sa + 0, Ko:].tolist() == [2 * sa + 2, -1, -1] and got[2 * sa + 2, Ko:].tolist() == [2 * sa + 0, -1, -1]
    for a in (0, 1, 3):                                       # scene 0: two finite others, one -1
        row = got[a, Ko:].tolist()
        assert row[2] == -1 and sorted(row[:2]) == sorted(set(range(sa)) - {a, 2}), row
    nbc = got[:, Ko:]
    assert (nbc != np.arange(S * sa)[:, None]).all()


# ================================================================================== solve
OUT_KEYS = ("x", "x_qp", "obj", "status", "iters", "alpha", "plan", "sel")


def outs(torch, s, A, n_obs, n_all, fill=0.0):
    Ko, Kn = s.n_selected(n_obs, n_all)
    nv = s.params.nv
    f8 = dict(dtype=torch.float64, device="cuda")
    i4 = dict(dtype=torch.int32, device="cuda")
    return dict(x=torch.full((A, nv), fill, **f8), x_qp=torch.full((A, nv), fill, **f8), obj=torch.full((A,), fill, **f8),
                status=torch.full((A, 2), -7, **i4), iters=torch.full((A, 2), -7, **i4), alpha=torch.full((A, 20), fill, **f8),
                plan=torch.full((A, N, 2), fill, **f8), sel=torch.full((A, Ko + Kn), -7, **i4))


def solve_dev(torch, s, b, rows, ob, nb, agent_offset=0, nbr_plan=None, fill=0.0):
    """solve_device of batch rows `rows` against the tables ob / nb; the outputs on the host."""
    A = rows.stop - rows.start
    o = outs(torch, s, A, 0 if ob is None else ob.shape[0], nb.shape[0], fill)
    x0 = dev(torch, b["x0"][rows])
    s.solve_device(x0, dev(torch, b["ref"][rows]), dev(torch, b["foot"][rows]), dev(torch, ob), dev(torch, nb), o,
                   agent_offset=agent_offset, alpha_buf=x0.clone(), nbr_plan=dev(torch, nbr_plan))
    torch.cuda.synchronize()
    return host(o)


def per_scene_solve(torch, u, b, S, sa, so, plan=None):
    parts = []
    for s in range(S):
        a, o = slice(s * sa, (s + 1) * sa), slice(s * so, (s + 1) * so)
        r = solve_dev(torch, u, b, a, b["obstacles"][o], b["nbr_state"][a], nbr_plan=None if plan is None else plan[a])
        r["sel"] = rebase(r["sel"], min(u.params.K_obs, so), s * so, s * sa)
        parts.append(r)
    return {k: np.concatenate([p[k] for p in parts]) for k in OUT_KEYS}


def assert_same(got, want, rows=None, what=""):
    for k in OUT_KEYS:
        g = got[k] if rows is None else got[k][rows]
        assert np.array_equal(g, want[k], equal_nan=True), (what, k)


@gpu
@pytest.mark.parametrize("mode", ["plans_off", "plans_on", "plan_selection"])
def test_solve_equals_per_scene_solve(mode):
    """4 scenes x 4 agents, 3 + 3 rows: every output of the scene-batched solve_device, and of the host path
    srb_solve_batch, is bitwise that of the four unsegmented solves (sel re-based)."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 4, 4, 5, 3, 3
    b = scene_batch(S, sa, so, seed=7)
    plan = None if mode == "plans_off" else plans_of(b, 2)
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so), plan_selection=mode == "plan_selection")
    u = new_solver(Ko, Kn, S * sa, plan_selection=mode == "plan_selection")
    got = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"], nbr_plan=plan)
    want = per_scene_solve(torch, u, b, S, sa, so, plan)
    assert_same(got, want, what="device")
    assert (got["iters"] > 0).all() and np.isfinite(got["x"]).all()              # real solves, not early exits
    if mode == "plans_on":                                    # the plans do reach the rows: another result than without
        off = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"])
        assert not np.array_equal(off["x"], got["x"])
    h = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"], alpha_buf=b["x0"], nbr_plan=plan)
    h["alpha"] = h["alpha"].reshape(S * sa, 20)
    assert_same(h, want, what="host")
    s.close(); u.close()


@gpu
def test_isolation_of_scene_0():
    """Every obstacle and every agent of the other scenes moved onto scene 0's agents: scene 0's sel and outputs do
    not change by a bit -- and with scenes off the same move does change sel, so the test can fail."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 4, 4, 5, 3, 3
    b = scene_batch(S, sa, so, seed=8)
    m = {k: v.copy() for k, v in b.items()}
    p0 = b["nbr_state"][:sa, :2]
    m["obstacles"][so:] = p0[np.arange((S - 1) * so) % sa]
    m["nbr_state"][sa:, :2] = p0[np.arange((S - 1) * sa) % sa]
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    a = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"])
    c = solve_dev(torch, s, m, slice(0, S * sa), m["obstacles"], m["nbr_state"])
    for k in OUT_KEYS:
        assert np.array_equal(a[k][:sa], c[k][:sa]), k
    s.set_scenes(0, 0)
    sa0, _, _ = select(torch, s, b["x0"], b["obstacles"], b["nbr_state"])
    sc0, _, _ = select(torch, s, m["x0"], m["obstacles"], m["nbr_state"])
    assert not np.array_equal(sa0[:sa], sc0[:sa])
    s.close()


@gpu
def test_shard_inside_scenes_equals_the_full_batch():
    """Team 3, a shard of 5 agents from agent_offset 4: it starts and ends inside a scene."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 3, 3, 5, 3, 2
    b = scene_batch(S, sa, so, seed=9, duplicates=True)
    plan = plans_of(b, 3)
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    for pl in (None, plan):
        full = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"], nbr_plan=pl)
        sh = solve_dev(torch, s, b, slice(4, 9), b["obstacles"], b["nbr_state"], agent_offset=4, nbr_plan=pl)
        assert_same(full, sh, rows=slice(4, 9), what="shard")
    s.set_option("plan_selection", 1)
    f, _, _ = select(torch, s, b["x0"], b["obstacles"], b["nbr_state"], nbr_plan=plan)
    g, _, _ = select(torch, s, b["x0"][4:9], b["obstacles"], b["nbr_state"], agent_offset=4, nbr_plan=plan)
    assert np.array_equal(f[4:9], g)
    s.close()


@gpu
def test_off_means_off():
    """set_scenes(0, 0) after use: the one-team results of a fresh context, bitwise."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 4, 4, 5, 3, 3
    b = scene_batch(S, sa, so, seed=11)
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    on = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"])
    s.set_scenes()
    assert s.scenes == (0, 0)
    off = solve_dev(torch, s, b, slice(0, S * sa), b["obstacles"], b["nbr_state"])
    u = new_solver(Ko, Kn, S * sa)
    want = solve_dev(torch, u, b, slice(0, S * sa), b["obstacles"], b["nbr_state"])
    assert_same(off, want)
    assert not np.array_equal(on["sel"], off["sel"])          # one team does select across the scenes
    s.close(); u.close()


# ================================================================================== metrics and rollout
METRICS = ("d_obs", "d_agent", "min_d_obs", "min_d_agent", "fail_cycle", "distance_to_fail")


def metrics_call(torch, s, state, ob, nb, n_agents, agent_offset, c, m):
    """srb_sim_metrics_device at cycle c (c_first 0) for `n_agents` rows of state against the tables ob / nb."""
    dp = lambda t: None if t is None else ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._dp)
    ip = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), srbnmpc._ip)
    sim = srbnmpc.Sim(state=dp(state), c_first=0, obstacles=dp(ob), nbr_state=dp(nb), n_obs=0 if ob is None else ob.shape[0],
                      n_all=0 if nb is None else nb.shape[0], agent_offset=agent_offset, d_obs=dp(m["d_obs"]),
                      d_agent=dp(m["d_agent"]), min_d_obs=dp(m["min_d_obs"]), min_d_agent=dp(m["min_d_agent"]),
                      fail_cycle=ip(m["fail_cycle"]), distance_to_fail=dp(m["distance_to_fail"]))
    rc = srbnmpc.lib().srb_sim_metrics_device(s._h, n_agents, ctypes.byref(sim), c, s._stream(None))
    torch.cuda.synchronize()
    return rc


def metric_buffers(torch, A):
    z = lambda dt: torch.full((A,), -7, dtype=dt, device="cuda")
    return {k: z(torch.int32 if k == "fail_cycle" else torch.float64) for k in METRICS}


@gpu
@pytest.mark.parametrize("sa,so", [(3, 6), (20, 6), (3, 0)])
def test_metrics_equal_per_scene_metrics(sa, so):
    """5 scenes x 3 agents: the 16-agent blocks of the unsegmented kernel would straddle scenes.  Two cycles (the
    running minima and fail_cycle carry over), against per-scene calls of the unsegmented kernel on views of the
    same buffers; then a shard that starts and ends inside a scene.  Team 20 is more than one block a scene."""
    torch = _need_gpu()
    S = 5
    b = scene_batch(S, sa, so, seed=12 + sa)
    if so:
        b["obstacles"][0] = b["x0"][0, [0, 2]] + [0.1, 0.0]   # agent 0 starts inside the fail radius
    rng = np.random.default_rng(5)
    s = new_solver(1, 1, S * sa, scenes=(sa, so))
    u = new_solver(1, 1, S * sa)
    ob = dev(torch, b["obstacles"]) if so else None
    got, want = metric_buffers(torch, S * sa), metric_buffers(torch, S * sa)
    for c in (0, 1):
        st = b["x0"].copy()
        st[:, [0, 2]] += c * rng.normal(0, 0.4, (S * sa, 2))
        if c == 1:
            st[1, 0] = np.nan                                  # a NaN row never wins
        state = dev(torch, st)
        nb = dev(torch, st[:, [0, 2, 1, 3]])
        assert metrics_call(torch, s, state, ob, nb, S * sa, 0, c, got) == 0
        for k in range(S):
            a, o = slice(k * sa, (k + 1) * sa), slice(k * so, (k + 1) * so)
            assert metrics_call(torch, u, state[a], ob[o] if so else None, nb[a], sa, 0, c,
                                {n: v[a] for n, v in want.items()}) == 0
        for n in METRICS:
            assert np.array_equal(got[n].cpu().numpy(), want[n].cpu().numpy(), equal_nan=True), (c, n)
    if so:
        fc = got["fail_cycle"].cpu().numpy()
        assert (fc >= 0).any() and (fc < 0).any()             # the draw holds both cases
    # the shard: rows 4 .. 8 of the last cycle's state, first cycle of fresh buffers
    sh, ref = metric_buffers(torch, 5), metric_buffers(torch, S * sa)
    assert metrics_call(torch, s, state[4:9], ob, nb, 5, 4, 0, sh) == 0
    assert metrics_call(torch, s, state, ob, nb, S * sa, 0, 0, ref) == 0
    for n in METRICS:
        assert np.array_equal(sh[n].cpu().numpy(), ref[n].cpu().numpy()[4:9], equal_nan=True), n
    s.close(); u.close()


RES_KEYS = ("traj", "status", "iters", "state") + METRICS


@gpu
@pytest.mark.parametrize("plans", [False, True])
def test_rollout_equals_per_scene_rollouts(plans):
    """3 scenes x 4 agents, 6 obstacles each, 3 cycles: the scene-batched Rollout.run(3) against three whole-team
    rollouts, step() x 3 against run(3), and scene_results() against numpy on results()."""
    torch = _need_gpu()
    S, sa, so, Ko, Kn, T = 3, 4, 6, 3, 3, 3
    b = workload.make_scenes(S, sa, N, C, seed=13, n_obs=so)
    s = new_solver(Ko, Kn, S * sa, scenes=(sa, so))
    u = new_solver(Ko, Kn, S * sa)
    f8 = torch.float64

    def roll(solver, rows, orows, mode="run"):
        r = srbnmpc.Rollout(solver, dev(torch, b["goal"][rows], f8), phase=dev(torch, b["phase"][rows], torch.int32),
                            plans=plans, obstacles=dev(torch, b["obstacles"][orows], f8))
        r.reset(dev(torch, b["x0"][rows], f8))
        if mode == "run":
            r.run(T)
        else:
            for _ in range(T):
                r.step()
        res = host(r.results())
        sr = host(r.scene_results()) if solver.scenes[0] else None
        torch.cuda.synchronize()
        return res, sr

    got, sr = roll(s, slice(0, S * sa), slice(0, S * so))
    parts = [roll(u, slice(k * sa, (k + 1) * sa), slice(k * so, (k + 1) * so))[0] for k in range(S)]
    for k in RES_KEYS:
        axis = 1 if k in ("traj", "status", "iters") else 0
        assert np.array_equal(got[k], np.concatenate([p[k] for p in parts], axis)), k
    assert got["traj"].shape == (T + 1, S * sa, 4) and not np.array_equal(got["traj"][0], got["traj"][T])
    stepped, _ = roll(s, slice(0, S * sa), slice(0, S * so), "step")
    for k in RES_KEYS:
        assert np.array_equal(got[k], stepped[k]), k
    assert sr["n_scenes"] == S and sr["scene_agents"] == sa
    assert np.array_equal(sr["min_d_agent"], got["min_d_agent"].reshape(S, sa).min(1))
    assert np.array_equal(sr["min_d_obs"], got["min_d_obs"].reshape(S, sa).min(1))
    assert np.array_equal(sr["n_failed"], (got["fail_cycle"].reshape(S, sa) >= 0).sum(1))
    st = got["status"]
    bad = ~(np.isin(st[..., 0], (0, 4)) & (st[..., 1] == 0))
    assert np.array_equal(sr["n_not_converged"], bad.reshape(T, S, sa).sum((0, 2)))
    assert (got["min_d_obs"] >= 0.0).all() and (got["traj"][0][:, [0, 2]] == b["x0"][:, [0, 2]]).all()
    s.close(); u.close()


# ================================================================================== refusals
@gpu
def test_refusals_by_name_and_nothing_is_launched():
    torch = _need_gpu()
    S, sa, so, Ko, Kn = 3, 3, 5, 3, 2
    b = scene_batch(S, sa, so, seed=14)
    s = new_solver(Ko, Kn, 16, scenes=(sa, so))
    lib = srbnmpc.lib()
    err = lambda: lib.srb_last_error().decode()
    # the setter's own refusals leave the setting as it was
    for bad, word in (((-1, 0), "negative"), ((3, -2), "negative"), ((0, 5), "scene_agents == 0")):
        assert lib.srb_ctx_set_scenes(s._h, *bad) == -1 and word in err()
        with pytest.raises(RuntimeError, match=word):
            s.set_scenes(*bad)
    a_, o_ = ctypes.c_int(), ctypes.c_int()
    assert lib.srb_ctx_scenes(s._h, ctypes.byref(a_), ctypes.byref(o_)) == 0 and (a_.value, o_.value) == (sa, so) == s.scenes

    A = S * sa
    cases = [("is not a multiple of scene_agents", dict(nb=b["nbr_state"][:A - 2], rows=slice(0, 4))),
             ("!= scenes * scene_obs", dict(ob=b["obstacles"][:S * so - 1])),
             ("beyond the last scene", dict(rows=slice(0, 4), agent_offset=6))]
    for word, kw in cases:
        ob, nb = kw.get("ob", b["obstacles"]), kw.get("nb", b["nbr_state"])
        rows, off = kw.get("rows", slice(0, A)), kw.get("agent_offset", 0)
        n = rows.stop - rows.start
        # the device solve: every output keeps its sentinel
        with pytest.raises(RuntimeError, match=re.escape(word)):
            solve_dev(torch, s, b, rows, ob, nb, agent_offset=off, fill=-7.0)
        o = outs(torch, s, n, ob.shape[0], nb.shape[0], fill=-7.0)
        x0 = dev(torch, b["x0"][rows])
        with pytest.raises(RuntimeError, match=re.escape(word)):
            s.solve_device(x0, dev(torch, b["ref"][rows]), dev(torch, b["foot"][rows]), dev(torch, ob), dev(torch, nb), o,
                           agent_offset=off, alpha_buf=x0.clone())
        torch.cuda.synchronize()
        assert all((v == -7).all().item() for v in o.values()), word
        # the selection alone, the metrics and the host path
        sel = torch.full((n, sum(s.n_selected(ob.shape[0], nb.shape[0]))), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match=re.escape(word)):
            s.select_device(x0, dev(torch, ob), dev(torch, nb), sel, agent_offset=off)
        torch.cuda.synchronize()
        assert (sel == -7).all().item()
        m = metric_buffers(torch, n)
        assert metrics_call(torch, s, dev(torch, b["x0"][rows]), dev(torch, ob), dev(torch, nb), n, off, 0, m) == -1
        assert word in err() and all((v == -7).all().item() for v in m.values())
        with pytest.raises(RuntimeError, match=re.escape(word)):
            s.solve(b["x0"][rows], b["ref"][rows], b["foot"][rows], ob, nb, agent_offset=off)

    # the rollout: n_agents is not a multiple of scene_agents (Rollout.run says so itself; the C driver by name)
    n = 5
    r = srbnmpc.Rollout(s, dev(torch, b["goal"][:n]), obstacles=dev(torch, b["obstacles"][:so]))
    r.reset(dev(torch, b["x0"][:n]))
    with pytest.raises(ValueError, match="multiple of scene_agents"):
        r.run(1)
    r._reserve(1)
    for t in (r.out["x"], r.traj, r.x0, r.last_state):
        t.fill_(-7)
    o = r.out
    dp = lambda v: None if v is None else ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._dp)
    ip = lambda v: ctypes.cast(ctypes.c_void_p(v.data_ptr()), srbnmpc._ip)
    bat = srbnmpc.Batch(None, None, None, dp(r.obstacles), None, so, n, 0, None, dp(o["x"]), dp(o["obj"]), ip(o["status"]),
                        ip(o["iters"]), None, dp(o["alpha"]), None, 0, None, None)
    assert lib.srb_rollout_device(s._h, n, ctypes.byref(bat), ctypes.byref(r._sim()), 1, s._stream(None)) == -1
    assert "not a multiple of scene_agents" in err()
    torch.cuda.synchronize()
    assert all((t == -7).all().item() for t in (r.out["x"], r.traj, r.x0, r.last_state))
    with pytest.raises(ValueError, match="whole number of scenes"):
        r.scene_results()

    # after the refusals the context solves as if nothing had happened
    got = solve_dev(torch, s, b, slice(0, A), b["obstacles"], b["nbr_state"])
    u = new_solver(Ko, Kn, A)
    want = per_scene_solve(torch, u, b, S, sa, so)
    assert_same(got, want)
    s.close(); u.close()
