"""Multi-GPU sharding for the agent batch (one process per GPU, torch.distributed).

Agents are independent given the neighbour snapshot (src/A1_Sim.cpp:181 reads the
neighbour state once per MPC call, include/shared_structs.hpp:94), so the batch shards
agent-major in contiguous blocks.  The only exchange is the neighbour snapshot: each rank
all-gathers the [x, y, xdot, ydot] rows of every agent (32 B per agent; RCCL over xGMI
when the backend is "nccl", gloo in the CPU tests) before the solve; the kNN and the
inter-agent CBF rows then run locally on each GPU.

Ranks exchange solutions only as plans, and only when asked to: PlanExchange all-gathers each
agent's predicted CoM positions ([N, 2], 16 N bytes per agent) into the [n_total, N, 2] table that
srb_batch.nbr_plan takes -- once per cycle from the previous cycle's plans (shift_plans), or once
per outer round of BatchSolver.solve_coupled_device.  Without a plan table the inter-agent rows
are the constant-velocity guess from the snapshot and no solution crosses ranks.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_range(n_total: int, world: int, rank: int):
    """Contiguous agent-major block of rank `rank` (sizes differ by at most one)."""
    lo = (n_total * rank) // world
    hi = (n_total * (rank + 1)) // world
    return lo, hi


class NeighbourExchange:
    """The per-cycle all-gather of the [n_local, 4] neighbour-state rows of every rank into
    one [n_total, 4] table in global agent order, with every buffer allocated once: each
    rank's rows go into a padded [cmax, 4] slot of one flat receive buffer
    (all_gather_into_tensor: a single RCCL call, no per-step list or torch.cat).  With equal
    shards (n_total % world == 0) the receive buffer IS the table; otherwise the padding is
    squeezed out by one index_select into a preallocated table.  `width` is the row length
    (4: the neighbour snapshot)."""

    def __init__(self, n_total: int, world: int, rank: int, device, dtype=None, force_collective: bool = False,
                 width: int = 4):
        """force_collective: run the all-gather even with one rank (tests: the RCCL path on one GPU)."""
        import torch as _t
        dtype = dtype or _t.float64
        self.n_total, self.world, self.rank = n_total, world, rank
        self.width = width = int(width)
        self.force = bool(force_collective)
        self.counts = [shard_range(n_total, world, r)[1] - shard_range(n_total, world, r)[0] for r in range(world)]
        self.cmax = max(self.counts)
        self.send = _t.zeros((self.cmax, width), dtype=dtype, device=device)
        self.recv = _t.zeros((world * self.cmax, width), dtype=dtype, device=device)
        self.equal = all(c == self.cmax for c in self.counts)
        if not self.equal:
            rows = [r * self.cmax + i for r in range(world) for i in range(self.counts[r])]
            self.rows = _t.as_tensor(rows, dtype=_t.long, device=device)
            self.table = _t.zeros((n_total, width), dtype=dtype, device=device)
        self.out = self.recv if self.equal else self.table     # the [n_total, width] table wait() returns
        # gloo (CPU tests) has no all_gather_into_tensor on every torch build: list form there
        self.flat = dist.is_initialized() and dist.get_backend() != "gloo"

    def __call__(self, local_state: torch.Tensor) -> torch.Tensor:
        return self.start(local_state).wait()

    def start(self, local_state: torch.Tensor) -> "PendingExchange":
        """Issue the all-gather without waiting for it (async_op): the caller runs work that does not need
        the neighbour table -- the static-obstacle selection (bench.py) -- then .wait() on the handle.  With
        RCCL, wait() orders the caller's current stream after the collective without blocking the host, so
        the static selection kernel and the all-gather overlap on the GPU."""
        if self.world == 1 and not self.force:
            return PendingExchange(self, None, local_state)
        if local_state.shape[0] != self.counts[self.rank]:
            raise ValueError(f"rank {self.rank} holds {self.counts[self.rank]} agents, got {local_state.shape[0]} rows")
        self.send[:local_state.shape[0]].copy_(local_state)
        if self.flat:
            work = dist.all_gather_into_tensor(self.recv, self.send, async_op=True)
        else:
            work = dist.all_gather(list(self.recv.view(self.world, self.cmax, self.width).unbind(0)), self.send, async_op=True)
        return PendingExchange(self, work, None)


class PendingExchange:
    """An all-gather in flight (NeighbourExchange.start); wait() returns the [n_total, width] table."""

    def __init__(self, ex: NeighbourExchange, work, table):
        self.ex, self.work, self.table = ex, work, table

    def wait(self) -> torch.Tensor:
        if self.table is not None:
            return self.table
        self.work.wait()
        ex = self.ex
        if ex.equal:
            self.table = ex.recv
        else:
            torch.index_select(ex.recv, 0, ex.rows, out=ex.table)
            self.table = ex.table
        return self.table


class PlanExchange:
    """The all-gather of every rank's plans ([n_local, N, 2], BatchSolver's out["plan"]) into the
    [n_total, N, 2] table in global agent order that srb_batch.nbr_plan takes: NeighbourExchange at
    width 2N, equal or unequal shards, start() / wait() as there.

    Buffers.  A solve that is still in flight may be reading the table of the previous exchange while the
    next exchange runs, so this class owns TWO sets of send / receive / table buffers and alternates between
    them: the table one wait() returned is not written again until the start() after next.  Under the
    driver's ordering (solve_coupled_device: solve r reads table r, its plans go into start(r + 1), solve
    r + 1 reads table r + 1, all issued on one stream, and a context runs its solves in submission order)
    the solve that read the older table has finished before the second start() after it can copy into that
    set: that copy is stream-ordered after solve r + 1, which the context orders after solve r.  A caller
    that keeps a table across more than one further exchange must copy it.  With one rank and no forced
    collective the plans themselves are the table (no copy, no buffer)."""

    def __init__(self, n_total: int, world: int, rank: int, device, N: int, dtype=None,
                 force_collective: bool = False):
        self.N = int(N)
        self.sets = [NeighbourExchange(n_total, world, rank, device, dtype, force_collective, width=2 * self.N)
                     for _ in range(2)]
        self.turn = 0
        self.n_total = n_total

    def __call__(self, plan: torch.Tensor) -> torch.Tensor:
        return self.start(plan).wait()

    def start(self, plan: torch.Tensor) -> "PendingPlanExchange":
        if plan.dim() != 3 or plan.shape[1] != self.N or plan.shape[2] != 2 or not plan.is_contiguous():
            raise ValueError(f"plans must be a contiguous [n_local, {self.N}, 2] tensor, got {tuple(plan.shape)}")
        ex = self.sets[self.turn]
        self.turn ^= 1
        return PendingPlanExchange(ex.start(plan.view(plan.shape[0], 2 * self.N)), self.N)


class PendingPlanExchange:
    """A plan all-gather in flight (PlanExchange.start); wait() returns the [n_total, N, 2] table."""

    def __init__(self, pending: PendingExchange, N: int):
        self.pending, self.N = pending, N

    def wait(self) -> torch.Tensor:
        t = self.pending.wait()
        return t.view(t.shape[0], self.N, 2)


def shift_plans(table: torch.Tensor, grids: int) -> torch.Tensor:
    """Last cycle's plans as this cycle's table: `table` [n, N, 2] holds positions at grids 1..N of the
    previous cycle; the new cycle starts `grids` grids later, so its grid k is the old grid k + grids.  The
    first `grids` grids are dropped and the tail is extended along the last finite difference,
    p_{N+j} = p_N + j (p_N - p_{N-1}).  Pure torch, a new tensor; grids = 0 returns the plans unchanged."""
    n, N, _ = table.shape
    g = int(grids)
    if g < 0:
        raise ValueError("grids must be >= 0")
    if N < 2:
        raise ValueError("shift_plans needs N >= 2")
    out = torch.empty_like(table)
    keep = max(N - g, 0)
    if keep:
        out[:, :keep] = table[:, g:]
    j = torch.arange(keep + g - N + 1, g + 1, dtype=table.dtype, device=table.device).view(1, -1, 1)
    out[:, keep:] = table[:, N - 1:N] + j * (table[:, N - 1:N] - table[:, N - 2:N - 1])
    return out


def gather_states(local_state: torch.Tensor, n_total: int, world: int) -> torch.Tensor:
    """One-shot form of NeighbourExchange (allocates its buffers per call)."""
    if world == 1:
        return local_state
    return NeighbourExchange(n_total, world, dist.get_rank(), local_state.device, local_state.dtype)(local_state)
