"""bench.py's multi-GPU launch path on CPU (VERDICT r02 "bench.py --gpus N is parsed and
ignored"): `python bench.py --gpus 2` without a launcher must start two ranks itself, and a
launcher whose WORLD_SIZE disagrees with --gpus must make it exit non-zero -- it can never
print n_gpus: 1 for a 2-GPU request.  --plumbing runs the launch / barrier / all-reduce path
on gloo without a GPU or a solve."""
import json
import os
import subprocess
import sys

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _env():
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e["OMP_NUM_THREADS"] = "1"
    return e


def test_bench_gpus2_spawns_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--plumbing", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks_reporting"] == 2 and line["plumbing"] is True
    assert "rank 0/2 reporting" in r.stderr and "rank 1/2 reporting" in r.stderr


def test_bench_world_size_mismatch_exits_nonzero():
    e = _env()
    e.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--plumbing"], capture_output=True, text=True,
                       timeout=120, env=e, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_dump_outputs_writes_float64_arrays_and_caps_by_a_seeded_row_sample(tmp_path, monkeypatch):
    """--dump-outputs: every output tensor as <name>.npy in float64 (None entries left out); beyond the
    size limit all arrays keep the same seeded sample of agent rows, identical from run to run."""
    import numpy as np
    import torch
    import bench
    out = dict(x_qp=None, x=torch.arange(40 * 6, dtype=torch.float64).reshape(40, 6),
               obj=torch.arange(40, dtype=torch.float64), status=torch.ones((40, 2), dtype=torch.int32))
    bench.dump_outputs(str(tmp_path / "a"), out, 1, 0)
    assert sorted(os.listdir(tmp_path / "a")) == ["obj.npy", "status.npy", "x.npy"]
    for k in ("x", "obj", "status"):
        a = np.load(tmp_path / "a" / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, out[k].numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * (6 + 1 + 2) * 8)      # room for 10 of the 40 rows
    bench.dump_outputs(str(tmp_path / "b"), out, 1, 0)
    bench.dump_outputs(str(tmp_path / "c"), out, 1, 0)
    idx = np.load(tmp_path / "b" / "sample_rows.npy").astype(int)
    assert idx.shape == (10,) and np.all(np.diff(idx) > 0) and idx.max() < 40
    for k in ("x", "obj", "status", "sample_rows"):
        b = np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(b, np.load(tmp_path / "c" / f"{k}.npy"))
        if k != "sample_rows":
            assert np.array_equal(b, out[k].numpy()[idx])
    bench.dump_outputs(str(tmp_path / "d"), out, 2, 1)                        # a shard of a 2-GPU run
    assert sorted(os.listdir(tmp_path / "d"))[:1] == ["obj.rank1.npy"]
