"""GPU tests of the reduced factor and solves with the row broadcast folded into the FMA (SRB_DPP_FOLD: csrc/srb_gj.h
gj_invert_dpp_fold, csrc/srb_solve.h la_solve / mv_fold -- one v_fmac_f64_dpp row_newbcast where bc16() + fma() compiled
to v_mov_b64_dpp + v_fma_f64).

1. The two forms agree bit for bit: tools/ubench/dpp_fold_check.hip compiles both from the product headers into one
   binary and compares inverse, failure flag and solve result at (NZL, NZE, nz) = (8, 8, 3), (12, 12, 4), (12, 11, 11),
   (12, 12, 12), (16, 16, 16) on a well-conditioned SPD matrix, one with diagonal weights up to 1e12, one with a pivot
   <= 1e-14 (regularise on and off), an indefinite one and one with a NaN entry, with delta = 0 and delta != 0.  The test
   builds it with hipcc (a missing compiler is a failure, not a skip) and runs it once as a child process.
2. The NZL <= 16 instances tests/test_gpu_factor_chain.py does not launch (16_1_1, 8_1_4, 12_1_4_0_0_0, 16_1_4, 16_2_4,
   12_2_2, 16_2_2; with several waves every wave factors redundantly and the failure branch must stay uniform), at the
   shapes of tests/instance_cases.py, 8 agents, against the oracle by that file's rule: statuses equal, iteration counts
   equal, X, U, s within 1e-4, within 1e-6 where both sides end NLP OPTIMAL.  The instance is asserted first through
   BatchSolver.last_kernels().  These instances keep the bc16() + fma() text (srb_dpp_fold, csrc/srb_wave.h;
   profiles/dpp_fold_static.txt) and are run all the same.
3. The instances that take the form, 12_4_1_10_2_11 and 12_1_4_10_2_3 (cases `default` and `w4` of
   tests/test_gpu_factor_chain.py SHAPES): two solves of one batch on one context and a shard of it, bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import instance_cases as ic
import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import srbnmpc  # noqa: E402
from srbnmpc import workload  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NLP_TOL = 1e-4
POLISHED_TOL = 1e-6


# ---------------------------------------------------------------------------- 1. the forms, bit for bit
def test_folded_forms_equal_the_unfolded_ones_bit_for_bit(tmp_path):
    exe = str(tmp_path / "dpp_fold_check")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value",
                         os.path.join(ROOT, "tools", "ubench", "dpp_fold_check.hip"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-4000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert lines[-1] == "mismatches: 0", lines[-1]
    # every size ran its twelve cases, flagged the indefinite and the NaN matrix and saw NaNs in the NaN matrix's inverse
    sizes = [ln for ln in lines if ln.startswith("NZL=")]
    assert [ln.split(":")[0] for ln in sizes] == ["NZL=8 NZE=8 nz=3", "NZL=12 NZE=12 nz=4", "NZL=12 NZE=11 nz=11",
                                                 "NZL=12 NZE=12 nz=12", "NZL=16 NZE=16 nz=16"]
    for ln in sizes:
        assert "12 cases, 4 flagged not PD" in ln and ", 0 mismatches" in ln and " 0 NaN words" not in ln, ln


# ---------------------------------------------------------------------------- 2. the other NZL <= 16 instances
RUN_TIME = [(16, 1, 1), (8, 1, 4), (12, 1, 4), (16, 1, 4), (16, 2, 4), (12, 2, 2), (16, 2, 2)]
OTHERS = [(d + (0, 0, 0), sh) for d in RUN_TIME for sh in ic.LIP_RUN_TIME[d]]


def xus(N, x):
    x = np.asarray(x)
    return np.concatenate([x[..., :6 * N], x[..., -1:]], -1)


@pytest.mark.parametrize("dims,shape", OTHERS, ids=["%d_%d_%d-N%dC%dK%d" % (d[:3] + tuple(s)) for d, s in OTHERS])
def test_other_one_block_instances_match_the_oracle(dims, shape):
    N, C, K = shape
    Ko, Kn = ic.split_K(K)
    b, r = ic.lip_batch(shape), ic.lip_plain(shape)
    A = b["x0"].shape[0]
    assert 8 <= A <= 32
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        s.set_waves(dims[2])
        out = s.solve(b["x0"], b["ref"], b["foot"], b["obstacles"], b["nbr_state"])
        out = {k: np.array(v, copy=True) for k, v in out.items() if v is not None}
        assert s.last_kernels() == ("srb_nmpc_kernel_" + "_".join(map(str, dims)), ""), s.last_kernels()
        assert s.waves() == dims[2]
    finally:
        s.close()
    e = np.abs(xus(N, out["x"]) - xus(N, r["x"])).max(1)
    both = (out["status"][:, 1] == 0) & (r["status"][:, 1] == 0)
    print("max |X,U,s - oracle| per agent:", e.max(), "where both OPTIMAL:", e[both].max() if both.any() else None,
          "statuses", np.unique(out["status"], axis=0, return_counts=True),
          "agents with other counts", int((out["iters"] != r["iters"]).any(1).sum()),
          "largest count difference", int(np.abs(out["iters"] - r["iters"]).max()))
    np.testing.assert_array_equal(out["status"], r["status"])
    np.testing.assert_array_equal(out["iters"], r["iters"])
    assert e.max() < NLP_TOL, (int(np.argmax(e)), float(e.max()))
    assert both.any()
    assert e[both].max() < POLISHED_TOL, (int(np.argmax(e * both)), float(e[both].max()))


# ---------------------------------------------------------------------------- 3. the instances that take the form
# tests/test_gpu_factor_chain.py SHAPES `default` and `w4`: N, C, K_obs, K_nbr, agents, waves asked for, waves expected,
# instance, the shard's rows
FOLDED = {
    "default": (10, 2, 3, 8, 64, 1, 1, "12_4_1_10_2_11", slice(32, 64)),
    "w4": (10, 2, 3, 0, 8, 0, 4, "12_1_4_10_2_3", slice(4, 8)),
}
OUT_KEYS = ("x", "x_qp", "obj", "status", "iters", "sel")


@pytest.mark.parametrize("name", list(FOLDED))
def test_two_solves_and_a_shard_are_bit_equal(name):
    N, C, Ko, Kn, A, waves, want, inst, rows = FOLDED[name]
    b = workload.make_batch(A, N, C, seed=17 * N + C + Kn)
    s = srbnmpc.BatchSolver(srbnmpc.default_params(N, C, K_obs=Ko, K_nbr=Kn), A)
    try:
        s.set_waves(waves)
        outs = []
        for rw, off in ((slice(None), 0), (slice(None), 0), (rows, rows.start)):
            out = s.solve(b["x0"][rw], b["ref"][rw], b["foot"][rw], b["obstacles"], b["nbr_state"], agent_offset=off)
            outs.append({k: np.array(v, copy=True) for k, v in out.items() if v is not None})
            assert s.waves() == want
            assert s.last_kernels() == ("srb_nmpc_kernel_" + inst, ""), s.last_kernels()
    finally:
        s.close()
    o1, o2, part = outs
    assert (o1["status"][:, 1] == 0).any()
    assert set(o1) == set(o2)
    for k in o1:
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k
    for k in OUT_KEYS:
        assert np.array_equal(o1[k][rows], part[k], equal_nan=True), k
