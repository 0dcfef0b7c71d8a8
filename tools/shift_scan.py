#!/usr/bin/env python3
"""CPU scan for the exits of the NLP inertia-shift loop (oracle only, no GPU): which crowded batches hold a shifted
agent that leaves through `near && delta != 0` (ACCEPTABLE) or exhausts the 14 tries (KKTFAIL).

    python tools/shift_scan.py [--seeds 64] [--agents 32] [-N 10] [--threads 8]

Per (seed, Sw in {3e4, 1e5, 3e5, 1e6}) it prints the number of shifted agents and the agents of either exit; the
cases tests/shift_cases.py LIP_EXITS names come from its output.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "srb-cbf-nmpc_amd")):
    sys.path.insert(0, p)

import oracle  # noqa: E402
from srbnmpc import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("-N", type=int, default=10)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    near, tries = oracle.EXIT_RULES.index("near_shifted"), oracle.EXIT_RULES.index("tries")
    found = {near: 0, tries: 0}
    for seed in range(a.seeds):
        b = workload.make_batch(a.agents, a.N, 2, seed=seed, n_obs=int(round(80 * workload.arena_scale(a.agents) ** 2)))
        for Sw in (3e4, 1e5, 3e5, 1e6):
            r = oracle.solve_batch(oracle.params(a.N, 2, K_obs=3, K_nbr=8, use_nlp=1, Sw=Sw), b["x0"], b["ref"], b["foot"],
                                   b["obstacles"], b["nbr_state"], nthreads=a.threads, stats=True)
            st = r["stats"]
            hits = {k: np.nonzero(st["exit"] == k)[0].tolist() for k in (near, tries)}
            for k in hits:
                found[k] += len(hits[k])
            if hits[near] or hits[tries]:
                print(f"seed {seed} Sw {Sw:g}: shifted {int((st['failed'] > 0).sum())} near_shifted {hits[near]} "
                      f"tries {hits[tries]} statuses {r['status'][hits[near] + hits[tries], 1].tolist()}", flush=True)
    print(f"total: near_shifted {found[near]} agents, tries exhausted {found[tries]} agents "
          f"({a.seeds} seeds x 4 Sw, N = {a.N}, {a.agents} agents)")


if __name__ == "__main__":
    main()
