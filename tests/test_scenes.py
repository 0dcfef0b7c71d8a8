"""CPU tests of the scene partition (srb_ctx_set_scenes, workload.make_scenes, the per-scene reductions of
Rollout.scene_results): what needs no GPU.  The device side is tests/test_scenes_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import srbnmpc
from srbnmpc import rollout, workload


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+srb_ctx_set_scenes\s*\(\s*srb_ctx\s*\*\s*ctx\s*,\s*int\s+scene_agents\s*,\s*int\s+scene_obs\s*\)\s*;", code)
    assert re.search(r"int\s+srb_ctx_scenes\s*\(\s*srb_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*scene_agents\s*,\s*int\s*\*\s*scene_obs\s*\)\s*;", code)
    assert re.search(r"#define\s+SRB_ABI_VERSION\s+6\b", code)
    lib = ctypes.CDLL(srbnmpc.LIB_PATH)
    assert hasattr(lib, "srb_ctx_set_scenes") and hasattr(lib, "srb_ctx_scenes")
    assert lib.srb_abi_version() == 6 == srbnmpc.ABI_VERSION
    data = open(srbnmpc.LIB_PATH, "rb").read()
    for k in (b"srb_knn_scene_kernel", b"srb_knn_plan_scene_kernel", b"srb_sim_scene_metrics_kernel"):
        assert k in data, k


def test_null_context_is_refused_with_a_text():
    lib = srbnmpc.lib()
    assert lib.srb_ctx_set_scenes(None, 4, 20) == -1
    assert "null" in lib.srb_last_error().decode()
    a, o = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.srb_ctx_scenes(None, ctypes.byref(a), ctypes.byref(o)) == -1
    assert "null" in lib.srb_last_error().decode() and (a.value, o.value) == (7, 7)


# ------------------------------------------------------------------------------------------- make_scenes
S, TEAM, N, C, NOBS = 3, 5, 10, 2, 20


def test_make_scenes_shapes():
    b = workload.make_scenes(S, TEAM, N, C, seed=1, n_obs=NOBS)
    A = S * TEAM
    assert b["x0"].shape == (A, 4) and b["ref"].shape == (A, 4 * N) and b["foot"].shape == (A, N, 2, C)
    assert b["obstacles"].shape == (S * NOBS, 2) and b["nbr_state"].shape == (A, 4)
    assert b["goal"].shape == (A, 2) and b["phase"].shape == (A,) and b["phase"].dtype == np.int32
    assert all(np.isfinite(v).all() for v in b.values())
    # the snapshot rows are the starts in the get_lastState layout, the goal make_batch's at the team's arena
    assert np.array_equal(b["nbr_state"], b["x0"][:, [0, 2, 1, 3]])
    assert np.array_equal(b["goal"], np.tile(workload.GOAL * [workload.arena_scale(TEAM), 1.0], (A, 1)))
    sc = workload.arena_scale(TEAM)
    assert (b["x0"][:, 0] >= 0).all() and (b["x0"][:, 0] <= 9 * sc).all() and (np.abs(b["x0"][:, 2]) <= 2 * sc).all()
    z = workload.make_scenes(2, 3, 4, 4, seed=0, n_obs=0)
    assert z["obstacles"].shape == (0, 2) and z["foot"].shape == (6, 4, 2, 4)


def test_make_scenes_is_deterministic_per_seed():
    a, b = workload.make_scenes(S, TEAM, N, C, seed=5), workload.make_scenes(S, TEAM, N, C, seed=5)
    c = workload.make_scenes(S, TEAM, N, C, seed=6)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["x0"], c["x0"]) and not np.array_equal(a["obstacles"], c["obstacles"])
    # the scenes of one call are different draws
    assert not np.array_equal(a["x0"][:TEAM], a["x0"][TEAM:2 * TEAM])
    assert not np.array_equal(a["obstacles"][:20], a["obstacles"][20:40])


def test_scene_s_does_not_depend_on_n_scenes():
    a, b = workload.make_scenes(3, TEAM, N, C, seed=2, n_obs=NOBS), workload.make_scenes(7, TEAM, N, C, seed=2, n_obs=NOBS)
    for k in a:
        per = NOBS if k == "obstacles" else TEAM
        assert np.array_equal(a[k], b[k][:3 * per]), k


@pytest.mark.parametrize("team,clearance", [(5, 0.5), (16, 0.5), (4, 0.9)])
def test_starts_keep_the_clearance_within_their_scene(team, clearance):
    b = workload.make_scenes(4, team, 4, 2, seed=3, n_obs=NOBS, clearance=clearance)
    for s in range(4):
        p = b["x0"][s * team:(s + 1) * team][:, [0, 2]]
        ob = b["obstacles"][s * NOBS:(s + 1) * NOBS]
        assert np.sqrt(((p[:, None] - ob[None]) ** 2).sum(-1)).min() >= clearance
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) + np.eye(team) * 1e9
        assert d.min() >= clearance
    # without the rejection the same arena does put starts inside the radius: the rule is what keeps them out
    free = workload.make_scenes(4, team, 4, 2, seed=3, n_obs=NOBS, clearance=0.0)
    p, ob = free["x0"][:, [0, 2]].reshape(4, team, 2), free["obstacles"].reshape(4, NOBS, 2)
    assert np.sqrt(((p[:, :, None] - ob[:, None]) ** 2).sum(-1)).min() < clearance


def test_impossible_clearance_names_the_scene():
    with pytest.raises(ValueError, match=r"scene 0"):
        workload.make_scenes(2, 4, 4, 2, seed=0, clearance=100.0)


# ------------------------------------------------------------------------------------------- scene_results
def test_scene_reductions_equal_numpy_on_hand_made_metrics():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    S_, sa, T = 4, 3, 5
    A = S_ * sa
    res = dict(min_d_agent=rng.uniform(0, 3, A), min_d_obs=rng.uniform(0, 3, A),
               fail_cycle=rng.integers(-1, 3, A).astype(np.int32), status=rng.integers(0, 5, (T, A, 2)).astype(np.int32))
    res["fail_cycle"][:sa] = -1                               # a scene without a failure
    res["status"][:, sa:2 * sa] = [4, 0]                      # a scene whose solves all converged (QP_WARM, OPTIMAL)
    got = rollout.reduce_scenes({k: torch.as_tensor(v) for k, v in res.items()}, sa)
    assert got["n_scenes"] == S_ and got["scene_agents"] == sa
    assert np.array_equal(got["min_d_agent"].numpy(), res["min_d_agent"].reshape(S_, sa).min(1))
    assert np.array_equal(got["min_d_obs"].numpy(), res["min_d_obs"].reshape(S_, sa).min(1))
    assert np.array_equal(got["n_failed"].numpy(), (res["fail_cycle"].reshape(S_, sa) >= 0).sum(1))
    st = res["status"]
    bad = ~(np.isin(st[..., 0], (0, 4)) & (st[..., 1] == 0))
    assert np.array_equal(got["n_not_converged"].numpy(), bad.reshape(T, S_, sa).sum((0, 2)))
    assert got["n_failed"][0] == 0 and got["n_not_converged"][1] == 0 and got["n_not_converged"].sum() > 0
    with pytest.raises(ValueError, match="whole number of scenes"):
        rollout.reduce_scenes({k: torch.as_tensor(v) for k, v in res.items()}, 5)
