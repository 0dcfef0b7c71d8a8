"""dist.PlanExchange over gloo at world size 2 (CPU): every rank ends with the [n_total, N, 2] plan table in
global agent order, for equal and unequal shards, and again from the same object with changed plans -- the
table of the first exchange staying intact through the second (the two buffer sets)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

N = 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, n_total, q):
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "srb-cbf-nmpc_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from srbnmpc import dist as sdist
        g = torch.Generator().manual_seed(5)
        plans = torch.randn(n_total, N, 2, dtype=torch.float64, generator=g)      # the same on every rank
        lo, hi = sdist.shard_range(n_total, world, rank)
        ex = sdist.PlanExchange(n_total, world, rank, torch.device("cpu"), N)
        first = ex(plans[lo:hi].contiguous())
        ok = tuple(first.shape) == (n_total, N, 2) and bool(torch.equal(first, plans))
        changed = plans * 2.0 + 1.0
        second = ex(changed[lo:hi].contiguous())
        ok &= bool(torch.equal(second, changed))
        ok &= bool(torch.equal(first, plans))                    # not overwritten by the exchange after it
        ok &= first.data_ptr() != second.data_ptr()
        third = ex.start(plans[lo:hi].contiguous()).wait()       # the first set again, start() / wait() form
        ok &= bool(torch.equal(third, plans)) and bool(torch.equal(second, changed))
        # the width argument leaves the neighbour exchange as it was
        st = torch.randn(n_total, 4, dtype=torch.float64, generator=g)
        ok &= bool(torch.equal(sdist.NeighbourExchange(n_total, world, rank, torch.device("cpu"))(st[lo:hi]), st))
        bad = False
        try:
            ex(plans[lo:hi, :N - 1].contiguous())
        except ValueError:
            bad = True
        q.put((rank, ok and bad, hi - lo))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_total", [64, 65])
def test_plan_exchange_world2(n_total):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    assert sum(r[2] for r in res) == n_total
    assert all(r[1] for r in res), res


def test_plan_exchange_one_rank_passes_the_plans_through():
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "srb-cbf-nmpc_amd"))
    from srbnmpc import dist as sdist
    plans = torch.arange(5 * N * 2, dtype=torch.float64).view(5, N, 2)
    ex = sdist.PlanExchange(5, 1, 0, torch.device("cpu"), N)
    t = ex(plans)
    assert t.data_ptr() == plans.data_ptr() and tuple(t.shape) == (5, N, 2)
