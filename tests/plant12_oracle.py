"""numpy restatement of the disturbed plant of the SRB-12 rollout (csrc/srb12_plant.hip) on top of plant_oracle and
sim12_oracle.

step12() is one forward-Euler step of orc12_dynamics' map in the kernel's grouping, roll12() the four steps of a
cycle, plant_state12() srb12_plant_state_kernel (the state z + d that starts a cycle, and d), advance_plant12() both
kernels: plant_state12, then sim12_oracle.advance12 on it.  The generator is plant_oracle's (philox4x32_10, uniform,
kicks): counter (c, g, 0, 0) for the planar kicks, the LIP plant's draws, and (c, g, 1, 0) for the angular ones.

Every expression keeps the kernel's grouping (contraction off; division rounds correctly on both sides), so the
comparison with the device is assert_array_equal -- except what passes through the roll's cos / sin, which are not
correctly rounded on either side: Theta and omega of a rolled state.  p and v of a rolled state never see a
trigonometric value (p' = p + Ts v, v' = v + (Ts / m) sum f + Ts g) and stay bitwise, as does everything without a
roll.

How far a trigonometric error travels (roll_amplification): write e for the error of cos / sin, in the unit in
which sim12_oracle.TRIG_TOL bounds it where it passes through unscaled.  One step adds to omega the sum over the legs
of Ts Iw^-1 [r]x f = Ts Iw^-1 tau, tau the net torque sum_on r_l x f_l, with Iw^-1 = Rz (s Ib)^-1 Rz'.  An error e in
cos and in sin turns Rz by at most sqrt2 e in the 2-norm, and Rz enters twice, so one step's omega is off by at most
    g1 e,   g1 = 2 sqrt2 Ts |Ib^-1|_2 / s |tau|_2,   the largest over the agents and the steps.
Theta' = Theta + Ts Rz' omega adds Ts (sqrt2 |omega| e + the error of omega) a step.
  at_state 0: psi is the model's, an input.  Four steps add up: omega within 4 g1 e.  Theta within
      Ts (0 + 1 + 2 + 3) g1 e + 4 Ts sqrt2 |omega|_max e, and |omega|_max <= |omega_0| + 4 g1 / (2 sqrt2) (the same
      torque makes it), so within (0.26 + 0.35) g1 e + 0.25 |omega_0| e: both within (4 g1 + 1) e for a start that
      turns at no more than 4 rad/s.
  at_state 1: psi is the plant's own yaw (psi' = psi + Ts omega_z exactly: the third row of Rz is constant), so the
      error of omega after a step turns the next step's Rz by Ts times it: per step the error of omega grows to
      q = 1 + Ts g1 times itself plus g1 e, hence after four steps within g1 e (1 + q + q^2 + q^3).
  rebuilt inputs: where the footholds and the reference yaw are not the device's own arrays but sim12_oracle's
      (each within TRIG_TOL of the device's), a foothold off by e moves a lever arm by e, omega by
      g_f e = Ts |Ib^-1|_2 / s sum_on |f_l|_2 e a step, and a reference yaw off by e counts as another error of Rz:
      g1 is then 2 g1 + g_f.
The tolerance of a comparison is TRIG_TOL times that amplification (at least TRIG_TOL), computed from the magnitudes
of the data compared -- from the formulas above, not from an observed error.  p and v carry none of it.
"""
import numpy as np

import plant_oracle
import sim12_oracle

NDOMAIN = sim12_oracle.NDOMAIN


def _inv3(M):
    """orc12_dynamics' inv3 on stacks [A][3][3]: cofactors over one reciprocal of the determinant."""
    a, b, c, d, e, f, g, h, i = (M[:, r, q] for r in range(3) for q in range(3))
    A0, B0, C0 = e * i - f * h, -(d * i - f * g), d * h - e * g
    r = 1.0 / ((a * A0 + b * B0) + c * C0)
    X = np.empty_like(M)
    X[:, 0, 0] = A0 * r; X[:, 0, 1] = -(b * i - c * h) * r; X[:, 0, 2] = (b * f - c * e) * r
    X[:, 1, 0] = B0 * r; X[:, 1, 1] = (a * i - c * g) * r; X[:, 1, 2] = -(a * f - c * d) * r
    X[:, 2, 0] = C0 * r; X[:, 2, 1] = -(a * h - b * g) * r; X[:, 2, 2] = (a * e - b * d) * r
    return X


def world_inertia_inverse(psi, Ibs):
    """(R [A][3][3], Iw^-1 [A][3][3]) at the yaws psi [A] for the body inertias Ibs [A][3][3]: T = Rz Ibs, Iw = T Rz',
    every entry (a b + c d) + e f."""
    n = psi.shape[0]
    c, s = np.cos(psi), np.sin(psi)
    R = np.zeros((n, 3, 3))
    R[:, 0, 0] = c; R[:, 0, 1] = -s; R[:, 1, 0] = s; R[:, 1, 1] = c; R[:, 2, 2] = 1.0
    T, Iw = np.empty((n, 3, 3)), np.empty((n, 3, 3))
    for i in range(3):
        for j in range(3):
            T[:, i, j] = (R[:, i, 0] * Ibs[:, 0, j] + R[:, i, 1] * Ibs[:, 1, j]) + R[:, i, 2] * Ibs[:, 2, j]
    for i in range(3):
        for j in range(3):
            Iw[:, i, j] = (T[:, i, 0] * R[:, j, 0] + T[:, i, 1] * R[:, j, 1]) + T[:, i, 2] * R[:, j, 2]
    return R, _inv3(Iw)


def step12(z, psi, ph, Ts, tm, tg, Ibs, u, fp, ct):
    """One step z [A][12] -> [A][12] about the yaws psi [A] and positions ph [A][3]: tm = Ts / m [A], tg = -(Ts grav),
    u [A][4][3] the forces, fp [A][4][3] the footholds, ct [A][4] the contact flags."""
    n = z.shape[0]
    R, Iwi = world_inertia_inverse(psi, Ibs)
    fv, fw = np.zeros((n, 3)), np.zeros((n, 3))
    for l in range(4):
        on = ct[:, l] != 0
        r0, r1, r2 = fp[:, l, 0] - ph[:, 0], fp[:, l, 1] - ph[:, 1], fp[:, l, 2] - ph[:, 2]
        zero = np.zeros(n)
        S = [[zero, -r2, r1], [r2, zero, -r0], [-r1, r0, zero]]
        f = u[:, l]
        for i in range(3):
            fv[:, i] = np.where(on, fv[:, i] + tm * f[:, i], fv[:, i])
            acc = fw[:, i]
            for j in range(3):
                W = Ts * ((Iwi[:, i, 0] * S[0][j] + Iwi[:, i, 1] * S[1][j]) + Iwi[:, i, 2] * S[2][j])
                acc = acc + W * f[:, j]
            fw[:, i] = np.where(on, acc, fw[:, i])
    zn = np.empty_like(z)
    for i in range(3):
        zn[:, i] = z[:, i] + Ts * z[:, 6 + i]
        zn[:, 3 + i] = z[:, 3 + i] + (((Ts * R[:, 0, i]) * z[:, 9] + (Ts * R[:, 1, i]) * z[:, 10]) + (Ts * R[:, 2, i]) * z[:, 11])
        zn[:, 6 + i] = z[:, 6 + i] + fv[:, i]
        zn[:, 9 + i] = z[:, 9 + i] + fw[:, i]
    zn[:, 8] = zn[:, 8] + tg
    return zn


def body_tables(p, A, agent_offset=0, mass=None, inertia=None):
    """(m [A], Ibs [A][3][3]) of the plant's bodies: mass[g] or the model's, inertia[g] * Ib or Ib, entry by entry."""
    g = agent_offset + np.arange(A)
    m = np.full(A, p.mass) if mass is None else np.asarray(mass, dtype=np.float64)[g]
    sc = np.ones(A) if inertia is None else np.asarray(inertia, dtype=np.float64)[g]
    Ib = np.array(list(p.Ib), dtype=np.float64).reshape(3, 3)
    return m, sc[:, None, None] * Ib[None]


def roll12(p, state, x, xref, foot, contact, m, Ibs, at_state, steps=NDOMAIN, trace=False):
    """`steps` steps from state [A][12] under U_k of x [A][24N+1] with the footholds foot [A][N][4][3] and contact flags
    [A][N][4] of grids 0 .. steps - 1; the linearisation point is the plant's own state (at_state) or the model's: the
    start state, then xref [A][N][12] grid k - 1.  trace: the list of states after every step instead."""
    N, Ts = p.N, p.Ts
    z = np.array(state, dtype=np.float64).reshape(-1, 12)
    A = z.shape[0]
    x = np.asarray(x, dtype=np.float64)
    U = x[:, 12 * N:24 * N].reshape(A, N, 4, 3)
    tm, tg = Ts / m, -(Ts * p.grav)
    out = []
    for k in range(steps):
        ph = z if (at_state or k == 0) else xref[:, k - 1]
        z = step12(z, np.array(ph[:, 5]), np.array(ph[:, 0:3]), Ts, tm, tg, Ibs, U[:, k], foot[:, k], contact[:, k])
        out.append(z)
    return out if trace else z


def disturbance12(A, c, agent_offset=0, seed=0, kick_v=None, kick_p=None, kick_w=None, pushes=None):
    """d [A][12] of cycle c, state order: the planar kicks of counter (c, g, 0, 0), the angular ones of (c, g, 1, 0),
    then the pushes (cycle, agent, dv [P][6]) in table order."""
    g = agent_offset + np.arange(A)
    d = np.zeros((A, 12))
    if kick_v is not None or kick_p is not None:
        u = plant_oracle.kicks(seed, c, g)
        if kick_v is not None:
            b = np.asarray(kick_v, dtype=np.float64)[g]
            d[:, 6] = d[:, 6] + b * u[:, 0]
            d[:, 7] = d[:, 7] + b * u[:, 1]
        if kick_p is not None:
            b = np.asarray(kick_p, dtype=np.float64)[g]
            d[:, 0] = d[:, 0] + b * u[:, 2]
            d[:, 1] = d[:, 1] + b * u[:, 3]
    if kick_w is not None:
        u = angular_kicks(seed, c, g)
        b = np.asarray(kick_w, dtype=np.float64)[g]
        for i in range(3):
            d[:, 9 + i] = d[:, 9 + i] + b * u[:, i]
    if pushes is not None:
        cyc, agent, dv = (np.asarray(t) for t in pushes)
        for q in range(cyc.shape[0]):
            a = int(agent[q]) - agent_offset
            if int(cyc[q]) == c and 0 <= a < A:
                for i in range(3):
                    d[a, 6 + i] = d[a, 6 + i] + dv[q, i]
                    d[a, 9 + i] = d[a, 9 + i] + dv[q, 3 + i]
    return d


def angular_kicks(seed, c, rows):
    """u [len(rows)][4] of counter (c, g, 1, 0), key (seed low, seed high); the kernel uses columns 0 .. 2."""
    rows = np.asarray(rows, dtype=np.int64)
    M = plant_oracle.MASK
    ctr = np.stack([np.full_like(rows, int(c) & M), rows & M, np.ones_like(rows), np.zeros_like(rows)], -1)
    key = np.array([int(seed) & M, (int(seed) >> 32) & M], dtype=np.uint64)
    return plant_oracle.uniform(plant_oracle.philox4x32_10(ctr, key))


def plant_state12(p, c, state_prev, x, xref=None, foot=None, contact=None, agent_offset=0, seed=0, kick_v=None,
                  kick_p=None, kick_w=None, mass=None, inertia=None, at_state=False, pushes=None):
    """(state [A][12], d [A][12]) at the start of cycle c > c_first: state_prev started cycle c - 1, x is its solution
    and xref, foot, contact were its inputs (read by a roll only); the tables have n_all rows, agent a is row
    agent_offset + a."""
    x = np.asarray(x, dtype=np.float64)
    A = x.shape[0]
    if mass is not None or inertia is not None or at_state:
        m, Ibs = body_tables(p, A, agent_offset, mass, inertia)
        z = roll12(p, state_prev, x, np.asarray(xref), np.asarray(foot), np.asarray(contact), m, Ibs, at_state)
    else:
        z = sim12_oracle.next_state12(x)
    d = disturbance12(A, c, agent_offset, seed, kick_v, kick_p, kick_w, pushes)
    return z + d, d


def advance_plant12(p, c, state_prev, x, goal, vref, phase=None, gait="trot", xref=None, foot=None, contact=None,
                    **plant):
    """srb12_plant_state_kernel then srb12_sim_advance_plant_kernel at cycle c > c_first: sim12_oracle.advance12's dict
    on the plant's state, plus state [A][12] and dist [A][12]."""
    st, d = plant_state12(p, c, state_prev, x, xref, foot, contact, **plant)
    out = sim12_oracle.advance12(p.N, p.Ts, st, goal, vref, c, phase, gait)
    out.update(state=st, dist=d)
    return out


def roll_amplification(p, x, foot, contact, ph, at_state, inertia=None, rebuilt=False, steps=NDOMAIN):
    """The factor on sim12_oracle.TRIG_TOL by which Theta and omega of a rolled state may differ between two
    evaluations of cos / sin (the module docstring), from the data: x [A][24N+1], foot [A][N][4][3], contact [A][N][4],
    ph [A][steps][3] the linearisation positions, inertia [A] the factors on I_b (None: 1); rebuilt: foot and the
    reference yaw are a restatement's, not the device's own."""
    N = p.N
    x = np.asarray(x, dtype=np.float64)
    A = x.shape[0]
    U = x[:, 12 * N:24 * N].reshape(A, N, 4, 3)[:, :steps]
    on = (np.asarray(contact)[:, :steps] != 0)[..., None]
    r = np.asarray(foot)[:, :steps] - np.asarray(ph)[:, :steps, None, :]
    tau = np.linalg.norm((np.cross(r, U) * on).sum(2), axis=-1)                   # [A][steps]
    sc = np.ones(A) if inertia is None else np.asarray(inertia, dtype=np.float64)
    Ibi = np.linalg.norm(np.linalg.inv(np.array(list(p.Ib)).reshape(3, 3)), 2) / sc
    g1 = (2.0 * np.sqrt(2.0) * p.Ts * Ibi[:, None] * tau).max()
    if rebuilt:
        g1 = 2.0 * g1 + (p.Ts * Ibi[:, None] * (np.linalg.norm(U, axis=-1) * on[..., 0]).sum(2)).max()
    if not at_state:
        return steps * g1 + 1.0
    q = 1.0 + p.Ts * g1
    return max(g1 * sum(q ** k for k in range(steps)), 1.0)
