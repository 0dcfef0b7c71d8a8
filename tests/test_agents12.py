"""CPU tests of agent sizes in the SRB-12 mode (srb_agent_sizes through srb12_solve_batch_agents[_device],
srb12_sim_metrics_agents_device, srb12_rollout_agents_device): the references of tests/agents12_oracle.py against the
per-column KKT certificate, the conditions on their inputs that keep the GPU comparisons from passing vacuously, the
names, and the refusals and the Python layer's validation that need no context (tests/test_agents12_gpu.py then holds
the device against the references)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import agents12_oracle as ao
import plan12_oracle as po
import srbnmpc
from srbnmpc import srb12

NEW_NAMES = ("srb12_solve_batch_agents", "srb12_solve_batch_agents_device", "srb12_sim_metrics_agents_device",
             "srb12_rollout_agents_device")
EQ_TOL, PRIM_TOL, STAT_TOL = 1e-9, 1e-7, 1e-6              # test_srb12_oracle_kkt_certificate
OPTIMAL = np.array([4, 0])                                  # QP stage at the warm-start tolerance, NLP stage OPTIMAL


def _inside(cert):
    return cert["eq"] < EQ_TOL and cert["prim"] < PRIM_TOL and cert["stat_rel"] < STAT_TOL


def _moved(N, r, r0):
    return int((np.abs(r["x"][:, :12 * N] - r0["x"][:, :12 * N]).max(1) > 1e-4).sum())


# ================================================================================== the references
@pytest.mark.parametrize("shape", ao.SHAPES12)
def test_pad_references_converge_move_and_carry_the_per_column_certificate(shape):
    """(a) and (c): every reference solve is OPTIMAL, at least 3 agents move by more than 1e-4 in X against the answer
    without a table, every answer carries the certificate at the padded levels, and at the uniform levels at least
    one is beyond 1e-6 in stationarity or beyond the other thresholds."""
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    b, p, r0 = R["b"], R["p"], ao.reference(shape, "none")
    pad = ao.pad_table(A, seed)
    for what, tab in (("pad", np.full(A, ao.PAD_Q)), ("pad_table", pad)):
        r = ao.reference(shape, what)
        assert (r["status"] == OPTIMAL).all(), (what, r["status"].tolist())
        moved = _moved(N, r, r0)
        wrong = 0
        worst = dict(eq=0.0, prim=0.0, stat_rel=0.0)
        for a in range(A):
            sel = np.concatenate([po.select(p, b, a)[:Ko], ao.snapshot_nbr(p, b, a)])
            obs, eps = ao.rows_agents(p, b, a, None, sel, pad=tab)
            assert eps[:Ko].tolist() == [ao.pad_level(p.eps_obs, tab[a])] * Ko and (eps[Ko:] == p.eps_nbr).all()
            cert = po.certificate(p, b, a, obs, eps, r["x"][a])
            assert _inside(cert), (what, a, cert)
            worst = {k: max(v, cert[k]) for k, v in worst.items()}
            wrong += not _inside(po.certificate(p, b, a, obs, ao.levels12(p, Ko, sel, a), r["x"][a]))
        print(f"shape {shape} {what}: {moved} agents moved by more than 1e-4, worst certificate {worst}, {wrong} of {A} "
              f"beyond the thresholds at the uniform levels")
        assert moved >= 3 and wrong >= 1


@pytest.mark.parametrize("shape", ao.SHAPES12)
def test_uniform_radius_reference_converges_and_carries_the_per_column_certificate(shape):
    """(b): OPTIMAL everywhere and the certificate at the level (r + r)^2 on every neighbour column with a row."""
    N, Ko, Kn, A, gait, seed = shape
    R = po.reference(shape)
    b, p, r = R["b"], R["p"], ao.reference(shape, "rad")
    assert (r["status"] == OPTIMAL).all(), r["status"].tolist()
    rad = np.full(A, ao.RAD_R)
    for a in range(A):
        sel = np.concatenate([po.select(p, b, a)[:Ko], ao.snapshot_nbr(p, b, a)])
        obs, eps = ao.rows_agents(p, b, a, None, sel, rad=rad)
        assert (eps[Ko:][sel[Ko:] >= 0] == ao.pair_level(ao.RAD_R, ao.RAD_R)).all() and (eps[:Ko] == p.eps_obs).all()
        assert _inside(po.certificate(p, b, a, obs, eps, r["x"][a])), a


@pytest.mark.parametrize("shape", ao.SHAPES_D)
def test_two_radii_reference_converges_mixes_moves_and_discriminates(shape):
    """(d): every reference solve is OPTIMAL, at least 3 agents select rows of both classes, at least 3 move by more
    than 1e-4 in X against the answer at eps_nbr, every answer carries the certificate at the pair levels, and at
    least one fails it at the uniform level."""
    N, Ko, Kn, A, gait, seed = shape
    R = ao.reference(shape, "two")
    b, p, r, rad, sel = R["b"], R["p"], R["r"], R["rad"], R["sel"]
    assert (r["status"] == OPTIMAL).all() and (R["r0"]["status"] == OPTIMAL).all(), r["status"].tolist()
    assert (sel >= 0).all() and sel.shape == (A, min(Kn, A - 1))
    rr = rad[sel]
    both = int((rr.min(1) != rr.max(1)).sum())
    moved = _moved(N, r, R["r0"])
    wrong = 0
    for a in range(A):
        obs, eps = ao.rows_agents(p, b, a, None, sel[a], rad=rad)
        assert eps.tolist() == [ao.pair_level(rad[a], rad[i]) for i in sel[a]]
        cert = po.certificate(p, b, a, obs, eps, r["x"][a])
        assert _inside(cert), (a, cert)
        wrong += not _inside(po.certificate(p, b, a, obs, ao.levels12(p, 0, sel[a], a), r["x"][a]))
    print(f"shape {shape}: {both} agents with rows of both classes, {moved} moved by more than 1e-4, {wrong} of {A} beyond "
          f"the thresholds at the uniform level")
    assert both >= 3 and moved >= 3 and wrong >= 1


def test_clearance_selection_helper_differs_from_the_snapshot_selection():
    """The radii matter to the selection helper in the worlds the GPU tests use."""
    shape = ao.SHAPES_D[0]
    R = ao.reference(shape, "two")
    want = ao.nbr_clear_select(R["b"], R["rad"] * 4.0, shape[2])
    assert want.shape == R["sel"].shape and (want != R["sel"]).any()


# ================================================================================== names
def test_header_declares_and_library_exports_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "srbnmpc.h")).read()
    L = srb12._lib()
    for n in NEW_NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(L, n), n
    assert "#define SRB_ABI_VERSION 6\n" in hdr
    assert L.srb_abi_version() == 6 == srbnmpc.ABI_VERSION
    assert "The SRB-12 mode and the MPC_dist shims have no agent sizes" not in hdr
    for fn in (srb12.Solver12.solve, srb12.Solver12.solve_device, srb12.Solver12.solve_coupled_device):
        assert {"agent_rad", "agent_pad", "nbr_clearance"} <= set(inspect.signature(fn).parameters), fn
    assert {"agent_rad", "agent_pad", "agent_body", "nbr_clearance"} <= set(
        inspect.signature(srb12.Rollout12.__init__).parameters)


# ================================================================================== refusals without a context
def test_refusals_that_need_no_gpu():
    """The refusals of srb_agent_sizes are made by name (SRB_ERR_ARG = -1) with a NULL context, through each new
    entry point: nothing is launched."""
    lib = srb12._lib()
    err = lambda: lib.srb_last_error().decode()
    d = np.zeros(64)
    ci = np.zeros(64, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    iptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    G, B = srbnmpc.AgentSizes, srb12.Batch12

    def batch(nbr):
        b = B()
        if nbr:
            b.nbr_state, b.n_all = ptr(d), 4
        return b

    def sim(nbr):
        s = srb12.Sim12(); s.goal = ptr(d)
        if nbr:
            s.nbr_state, s.n_all = ptr(d), 4
        return s
    calls = (lambda ag, nbr: lib.srb12_solve_batch_agents(None, 1, ctypes.byref(batch(nbr)), None, None, None, ctypes.byref(ag)),
             lambda ag, nbr: lib.srb12_solve_batch_agents_device(None, 1, ctypes.byref(batch(nbr)), None, None, None,
                                                                 ctypes.byref(ag), None),
             lambda ag, nbr: lib.srb12_sim_metrics_agents_device(None, 1, ctypes.byref(sim(nbr)), None, ctypes.byref(ag), 0,
                                                                 None),
             lambda ag, nbr: lib.srb12_rollout_agents_device(None, 1, ctypes.byref(batch(nbr)), ctypes.byref(sim(nbr)), None,
                                                             None, None, ctypes.byref(ag), 1, None))
    for i, fn in enumerate(calls):
        for bad in (0, ctypes.sizeof(G) - 8, ctypes.sizeof(G) + 8, ctypes.sizeof(B)):
            ag = G(); ag.struct_size = bad
            assert fn(ag, True) == -1 and "srb_agent_sizes.struct_size" in err()
        for bad in (2, -1):
            assert fn(G(ptr(d), None, None, bad, None), True) == -1 and "srb_agent_sizes.clearance_selection: 0" in err()
        assert fn(G(None, ptr(d), None, 1, None), True) == -1 and "clearance_selection = 1 needs agent_rad" in err()
        assert fn(G(None, None, None, 0, iptr(ci)), True) == -1 and "collide_cycle needs agent_body" in err()
        if i < 3:            # (the rollout's neighbour table is the team itself)
            assert fn(G(ptr(d), None, None, 0, None), False) == -1 and "agent_rad needs a neighbour table" in err()
            assert fn(G(None, None, ptr(d), 0, None), False) == -1 and "agent_body needs a neighbour table" in err()
        # a good srb_agent_sizes: the refusal of the entry extended
        assert fn(G(ptr(d), ptr(d), ptr(d), 1, iptr(ci)), True) == -1 and "null argument" in err()
        assert fn(G(), False) == -1 and "null argument" in err()
    # what the extended entry points refuse comes through as well
    sz = srbnmpc.Sizes(None, None, 1)
    assert lib.srb12_solve_batch_agents_device(None, 1, ctypes.byref(B()), None, None, ctypes.byref(sz), ctypes.byref(G()),
                                               None) == -1 and "clearance_selection = 1 needs obs_eps" in err()
    mv = srbnmpc.Moving(None, 1, None)
    assert lib.srb12_solve_batch_agents(None, 1, ctypes.byref(B()), None, ctypes.byref(mv), None,
                                        ctypes.byref(G())) == -1 and "horizon_selection = 1 needs obs_vel" in err()
    b = B(); b.struct_size += 8
    assert lib.srb12_rollout_agents_device(None, 1, ctypes.byref(b), ctypes.byref(sim(True)), None, None, None,
                                           ctypes.byref(G()), 1, None) == -1 and "srb12_batch.struct_size" in err()
    s = sim(True); s.struct_size += 8
    assert lib.srb12_sim_metrics_agents_device(None, 1, ctypes.byref(s), None, ctypes.byref(G()), 0,
                                               None) == -1 and "srb12_sim.struct_size" in err()


def test_python_layer_validates_by_name_without_a_context():
    """The tables are checked before the library (or the context) is touched: a Solver12 that was never created
    serves.  nbr_clearance without agent_rad is the library's refusal, made by name before it touches the (null)
    context."""
    s = srb12.Solver12.__new__(srb12.Solver12)
    s.params, s._scenes, s._h = srb12.default_params(10, K_obs=1, K_nbr=2), (0, 0), None
    s.max_agents, s.device = 8, 0
    A, N, n_obs = 4, 10, 5
    x0, xref, foot = np.zeros((A, 12)), np.zeros((A, N, 12)), np.zeros((A, N, 4, 3))
    contact, ob, nb = np.zeros((A, N, 4), np.int32), np.zeros((n_obs, 2)), np.zeros((A, 4))
    for name in ("agent_rad", "agent_pad"):
        for bad in (np.zeros(A, np.float32), np.zeros((A, 1)), np.zeros(A + 1), np.zeros(2 * A)[::2], [1.0] * A):
            with pytest.raises(ValueError, match=f"{name} must be a contiguous float64 array"):
                s.solve(x0, xref, foot, contact, ob, nb, **{name: bad})
        with pytest.raises(ValueError, match=f"{name} must be finite"):
            s.solve(x0, xref, foot, contact, ob, nb, **{name: np.array([0.1, np.nan, 0.1, 0.1])})
    with pytest.raises(ValueError, match="agent_rad must be >= 0"):
        s.solve(x0, xref, foot, contact, ob, nb, agent_rad=np.array([0.1, -0.1, 0.1, 0.1]))
    with pytest.raises(RuntimeError, match="agent_rad needs a neighbour table") as e:
        s.solve(x0, xref, foot, contact, ob, None, agent_rad=np.zeros(0))
    assert "srbnmpc error -1:" in str(e.value)
    with pytest.raises(RuntimeError, match="clearance_selection = 1 needs agent_rad"):
        s.solve(x0, xref, foot, contact, ob, nb, nbr_clearance=True)
    with pytest.raises(RuntimeError, match="null argument"):                     # a negative pad is a valid pad
        s.solve(x0, xref, foot, contact, ob, nb, agent_pad=np.full(A, -0.1))
    q = srb12.Solver12.__new__(srb12.Solver12)
    q.params, q._scenes, q._h = srb12.default_params(10, K_obs=1, K_nbr=2, use_nlp=0), (0, 0), None
    with pytest.raises(ValueError, match="QP-only solve has no obstacle rows"):
        q.solve(x0, xref, foot, contact, ob, nb, agent_rad=np.ones(A))
    torch = pytest.importorskip("torch")
    t = lambda a: torch.as_tensor(a)
    out = dict(x=t(np.zeros((A, 241))), obj=t(np.zeros(A)), status=t(np.zeros((A, 2), np.int32)),
               iters=t(np.zeros((A, 2), np.int32)))
    args = (t(x0), t(xref), t(foot), t(contact), t(ob), t(nb))
    for name in ("agent_rad", "agent_pad"):
        for bad in (torch.zeros(A, dtype=torch.float32), torch.zeros(A + 1, dtype=torch.float64),
                    torch.zeros(2 * A, dtype=torch.float64)[::2], torch.zeros(A, 1, dtype=torch.float64)):
            with pytest.raises(ValueError, match=f"{name} must be"):
                s.solve_device(*args, out, **{name: bad})
            with pytest.raises(ValueError, match=f"{name} must be"):
                s.solve_coupled_device(*args, dict(out, plan=torch.zeros(A, N, 2, dtype=torch.float64)), outer=1,
                                       **{name: bad})
    with pytest.raises(ValueError, match="agent_rad must be >= 0"):
        s.solve_device(*args, out, agent_rad=torch.tensor([0.1, 0.2, -1.0, 0.3], dtype=torch.float64))
