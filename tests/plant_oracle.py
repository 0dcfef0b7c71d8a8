"""numpy restatement of the disturbed plant (csrc/srb_plant.hip), bit for bit, on top of sim_oracle.

philox4x32_10() is the counter-based generator of the kicks (Random123's known answers are in test_plant.py),
uniform() the exact word -> (-1, 1) conversion, lip() the discretisation of srb_capi.cpp's make_kparams operation
for operation, plant_state() the state z + d that starts a cycle and advance_plant() the whole
srb_sim_advance_plant_kernel: plant_state, then sim_oracle.advance and sim_oracle.shift4 on it.  Every expression
keeps the kernel's grouping (the kernel is compiled with contraction off; numpy's division rounds correctly, as the
device's does), so the comparison with the device is assert_array_equal.
"""
import numpy as np

import sim_oracle

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10: counter [..., 4], key [..., 2] (any integers, taken mod 2^32; broadcast) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(MASK)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (np.array(c[..., i]) for i in range(4))
    k0, k1 = np.array(k[..., 0]), np.array(k[..., 1])
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        n0, n1 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m, p1 & m
        n2, n3 = ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m, p0 & m
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def uniform(w):
    """((double)(int32_t)w + 0.5) * 2^-31 of uint32 words: exact, inside (-1, 1), never 0."""
    return (np.asarray(w, dtype=np.uint32).astype(np.int32).astype(np.float64) + 0.5) * 2.0 ** -31


def kicks(seed, c, rows):
    """u [len(rows)][4] of cycle c for the global rows `rows`: key (seed low, seed high), counter (c, g, 0, 0)."""
    rows = np.asarray(rows, dtype=np.int64)
    ctr = np.stack([np.full_like(rows, int(c) & MASK), rows & MASK, np.zeros_like(rows), np.zeros_like(rows)], -1)
    key = np.array([int(seed) & MASK, (int(seed) >> 32) & MASK], dtype=np.uint64)
    return uniform(philox4x32_10(ctr, key))


def _mm4(X, Y):
    """make_kparams' mm4 on stacks [A][4][4]: every entry s = 0; s += X[i][k] * Y[k][j], k = 0 .. 3."""
    Z = np.zeros_like(X)
    for i in range(4):
        for j in range(4):
            s = np.zeros(X.shape[0])
            for k in range(4):
                s = s + X[:, i, k] * Y[:, k, j]
            Z[:, i, j] = s
    return Z


def lip(grav, hcom, T):
    """(Ad [A][4][4], Bd [A][4][2]) of the LIP at the CoM heights hcom [A] (make_kparams, srb_capi.cpp:229-244)."""
    w2 = grav / np.asarray(hcom, dtype=np.float64)
    n = w2.shape[0]
    A, B, Ai = np.zeros((n, 4, 4)), np.zeros((n, 4, 2)), np.zeros((n, 4, 4))
    A[:, 0, 1] = 1; A[:, 1, 0] = w2; A[:, 2, 3] = 1; A[:, 3, 2] = w2
    B[:, 1, 0] = -w2; B[:, 3, 1] = -w2
    A2 = _mm4(A, A)
    A3 = _mm4(A2, A)
    eye = np.eye(4)[None]
    Ad = ((eye + A * T) + ((0.5 * A2) * T) * T) + (((A3 * T) * T) * T) / 6
    Ai[:, 0, 1] = 1.0 / w2; Ai[:, 1, 0] = 1.0; Ai[:, 2, 3] = 1.0 / w2; Ai[:, 3, 2] = 1.0
    M = _mm4(Ai, Ad - eye)
    Bd = np.zeros((n, 4, 2))
    for i in range(4):
        for j in range(2):
            s = np.zeros(n)
            for q in range(4):
                s = s + M[:, i, q] * B[:, q, j]
            Bd[:, i, j] = s
    return Ad, Bd


def roll4(Ad, Bd, z, U):
    """Four steps z <- Ad z + Bd u from z [A][4] under U [A][>= 4][2]: a row sum in index order, Ad's four terms then
    Bd's two, from the first product."""
    z = np.array(z, dtype=np.float64)
    for k in range(sim_oracle.NDOMAIN):
        u0, u1 = U[:, k, 0], U[:, k, 1]
        zn = np.empty_like(z)
        for i in range(4):
            zn[:, i] = ((((Ad[:, i, 0] * z[:, 0] + Ad[:, i, 1] * z[:, 1]) + Ad[:, i, 2] * z[:, 2]) +
                         Ad[:, i, 3] * z[:, 3]) + Bd[:, i, 0] * u0) + Bd[:, i, 1] * u1
        z = zn
    return z


def plant_state(N, Ts, grav, c, state_prev, x, agent_offset=0, seed=0, kick_v=None, kick_p=None, plant_hcom=None,
                pushes=None):
    """(state [A][4], d [A][4]) at the start of cycle c > c_first: state_prev [A][4] started cycle c - 1, x [A][nv] is
    its solution; the tables have n_all rows, agent a is row agent_offset + a; pushes = (cycle, agent, dv) or None.
    d = (dpx, dvx, dpy, dvy)."""
    x = np.asarray(x, dtype=np.float64)
    A = x.shape[0]
    g = agent_offset + np.arange(A)
    if plant_hcom is None:
        z = sim_oracle.next_state(x)
    else:
        Ad, Bd = lip(grav, np.asarray(plant_hcom, dtype=np.float64)[g], Ts)
        z = roll4(Ad, Bd, np.asarray(state_prev, dtype=np.float64).reshape(A, 4), x[:, 4 * N:6 * N].reshape(A, N, 2))
    d = np.zeros((A, 4))                                     # dpx, dvx, dpy, dvy
    if kick_v is not None or kick_p is not None:
        u = kicks(seed, c, g)
        if kick_v is not None:
            b = np.asarray(kick_v, dtype=np.float64)[g]
            d[:, 1] = d[:, 1] + b * u[:, 0]
            d[:, 3] = d[:, 3] + b * u[:, 1]
        if kick_p is not None:
            b = np.asarray(kick_p, dtype=np.float64)[g]
            d[:, 0] = d[:, 0] + b * u[:, 2]
            d[:, 2] = d[:, 2] + b * u[:, 3]
    if pushes is not None:
        cyc, agent, dv = (np.asarray(t) for t in pushes)
        for p in range(cyc.shape[0]):
            a = int(agent[p]) - agent_offset
            if int(cyc[p]) == c and 0 <= a < A:
                d[a, 1] = d[a, 1] + dv[p, 0]
                d[a, 3] = d[a, 3] + dv[p, 1]
    return z + d, d


def advance_plant(N, C, Ts, grav, vref, c, state_prev, x, goal, phase=None, **plant):
    """srb_sim_advance_plant_kernel at cycle c > c_first: sim_oracle.advance's dict on the plant's state, plus
    state [A][4], dist [A][4] and plan_table [A][N][2] (the shift of x, which the plant leaves alone)."""
    st, d = plant_state(N, Ts, grav, c, state_prev, x, **plant)
    out = sim_oracle.advance(N, C, Ts, st, goal, vref, c, phase)
    out.update(state=st, dist=d, plan_table=sim_oracle.shift4(N, x))
    return out
