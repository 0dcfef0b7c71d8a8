"""numpy restatement of the degraded neighbour link (csrc/srb_link.hip), bit for bit, on top of plant_oracle's Philox.

draws() gives the uniform words of a cycle's loss (third counter word 2) or noise (3) for a set of global rows,
new_state() the caller-owned state of a link (ring, held message, held cycle) filled with a sentinel, and update() one
cycle of srb_link_update_kernel over all rows: the message of cycle c into its ring slot, the arrival of the message of
c - delay, and the perceived tables.  Every expression keeps the kernel's grouping (the kernel is compiled with
contraction off), so the comparison with the device is assert_array_equal -- of the perceived tables, of the age and of
every state buffer.  The plan shift is sim_oracle.shift4's rule at 4 age grids instead of 4.
"""
import numpy as np

import plant_oracle
import sim_oracle

MASK = plant_oracle.MASK
LOSS, NOISE = 2, 3                       # the third counter word (the plants use 0 and 1)


def draws(seed, cycles, rows, word):
    """u [len(rows)][4]: key (seed low, seed high), counter (cycles[i] or the one cycle, rows[i], word, 0)."""
    rows = np.asarray(rows, dtype=np.int64)
    cyc = np.broadcast_to(np.asarray(cycles, dtype=np.int64), rows.shape)
    ctr = np.stack([cyc & MASK, rows & MASK, np.full_like(rows, word), np.zeros_like(rows)], -1)
    key = np.array([int(seed) & MASK, (int(seed) >> 32) & MASK], dtype=np.uint64)
    return plant_oracle.uniform(plant_oracle.philox4x32_10(ctr, key))


def tables(seed=0, delay=None, drop=None, noise_p=None, noise_v=None, max_delay=None, extrapolate=0, Ts=None):
    """The link's tables as update() takes them; max_delay defaults to the largest delay, Ts to the workload's."""
    from srbnmpc import workload
    if max_delay is None:
        max_delay = 0 if delay is None else int(np.max(delay))
    return dict(seed=int(seed), delay=delay, drop=drop, noise_p=noise_p, noise_v=noise_v, max_delay=int(max_delay),
                extrapolate=int(extrapolate), Ts=workload.TS if Ts is None else float(Ts))


def new_state(n_all, N, max_delay, fill=-7.0):
    """The link's state buffers, every entry `fill` (the device test fills its buffers with the same sentinel)."""
    S = max_delay + 1
    return dict(ring_state=np.full((S, n_all, 4), float(fill)), ring_plan=np.full((S, n_all, N, 2), float(fill)),
                held_state=np.full((n_all, 4), float(fill)), held_plan=np.full((n_all, N, 2), float(fill)),
                held_cycle=np.full(n_all, int(fill), np.int32))


def shift(P, m):
    """Plans P [n][N][2] shifted by m [n] grids each (m >= 0): grid k + m inside the horizon, beyond it
    last + (double)(k + m - N + 1) * (last - previous); m = sim_oracle.NDOMAIN is sim_oracle.shift4's rule."""
    n, N, _ = P.shape
    rows = np.arange(n)
    last = P[:, N - 1]
    e = last - P[:, N - 2]
    out = np.empty_like(P)
    for k in range(N):
        i = k + m
        inside = P[rows, np.minimum(i, N - 1)]
        beyond = last + (i - N + 1).astype(np.float64)[:, None] * e
        out[:, k] = np.where((i < N)[:, None], inside, beyond)
    return out


def update(c, c_first, truth_state, truth_plan, tab, link_state):
    """One cycle: (seen_state [n][4], seen_plan [n][N][2] or None, age [n] int32, the new link state).  truth_state
    [n][4] (x, y, xdot, ydot) and truth_plan [n][N][2] or None are the cycle's last_state and plan_table; link_state is
    not modified.  seen_plan is None where the kernel writes none: at c_first, or without a plan table."""
    st = {k: np.array(v) for k, v in link_state.items()}
    ts = np.asarray(truth_state, dtype=np.float64)
    n = ts.shape[0]
    rows = np.arange(n)
    D, Ts, seed = tab["max_delay"], tab["Ts"], tab["seed"]
    slots = D + 1
    with np.errstate(invalid="ignore", over="ignore"):
        msg = ts.copy()
        if tab["noise_p"] is not None or tab["noise_v"] is not None:
            u = draws(seed, c, rows, NOISE)
            if tab["noise_p"] is not None:
                msg[:, 0] = ts[:, 0] + tab["noise_p"] * u[:, 0]
                msg[:, 1] = ts[:, 1] + tab["noise_p"] * u[:, 1]
            if tab["noise_v"] is not None:
                msg[:, 2] = ts[:, 2] + tab["noise_v"] * u[:, 2]
                msg[:, 3] = ts[:, 3] + tab["noise_v"] * u[:, 3]
        plans = truth_plan is not None and c > c_first
        slot_c = (c - c_first) % slots
        st["ring_state"][slot_c] = msg
        if plans:
            st["ring_plan"][slot_c] = truth_plan
        if c == c_first:
            s, arrive = np.full(n, c), np.ones(n, bool)
        else:
            d = np.zeros(n, np.int64) if tab["delay"] is None else np.clip(np.asarray(tab["delay"], np.int64), 0, D)
            s = c - d
            arrive = s > c_first
            if tab["drop"] is not None:
                u0 = draws(seed, s, rows, LOSS)[:, 0]
                arrive &= ~(0.5 * u0 + 0.5 < tab["drop"])
        a = np.nonzero(arrive)[0]
        slot_s = (s[a] - c_first) % slots
        st["held_state"][a] = st["ring_state"][slot_s, a]
        if plans:
            st["held_plan"][a] = st["ring_plan"][slot_s, a]
        st["held_cycle"][a] = s[a]
        age = (c - st["held_cycle"]).astype(np.int32)
        h = st["held_state"]
        m = sim_oracle.NDOMAIN * age.astype(np.int64) if tab["extrapolate"] else np.zeros(n, np.int64)
        seen = h.copy()
        mv = m > 0
        dt = m.astype(np.float64) * Ts
        seen[mv, 0] = h[mv, 0] + h[mv, 2] * dt[mv]
        seen[mv, 1] = h[mv, 1] + h[mv, 3] * dt[mv]
        seen_plan = None
        if plans:
            seen_plan = shift(st["held_plan"], m)
            none = st["held_cycle"] == c_first                 # no plan held yet: constant velocity from the seen state
            for k in range(seen_plan.shape[1]):
                seen_plan[none, k] = seen[none, :2] + seen[none, 2:] * (Ts * float(k + 1))
    return seen, seen_plan, age, st


def run(c_first, truth_states, truth_plans, tab, N, fill=-7.0):
    """update() over consecutive cycles from a fresh state: truth_states [T][n][4], truth_plans [T][n][N][2] or None
    (its row 0 is never sent) -> list of (seen_state, seen_plan, age, link state) per cycle."""
    st = new_state(np.asarray(truth_states).shape[1], N, tab["max_delay"], fill)
    out = []
    for i, ts in enumerate(truth_states):
        r = update(c_first + i, c_first, ts, None if truth_plans is None else truth_plans[i], tab, st)
        st = r[3]
        out.append(r)
    return out
