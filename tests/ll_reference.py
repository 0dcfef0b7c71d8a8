"""Extended-precision reference of the low-level CLF-QP (test infrastructure only, plain numpy).

  ipm_ld       iSWIFT's predictor-corrector iteration (Prime.c:127-230, Auxilary.c kkt_initialize,
               computeresiduals, findsteplength, formrho, as the kernel's comments cite them; without
               the rounding-only sigma <= sigma_d branch, as the kernel and its oracle) in 80-bit
               np.longdouble.  Every Newton system is the dense unreduced
                   [P A' G'; A 0 0; G 0 -W] [dx; dy; dz] = [r1; r2; r3]
               solved by Gaussian elimination with partial pivoting written here in longdouble
               (np.linalg drops to fp64).  Nothing is eliminated and nothing is structured: it shares
               no linear algebra with the kernel (closed-form block factors + Schur complement) or
               with the fp64 oracle (dz eliminated, dense LU of the reduced system).
  epilogue_np  parse, swing PD, ddq, integration and swingInvKin of LowLevelCtrl::calcTorque from a
               given x, in numpy.
  clf_np       the CLF scalars V, LfV, cc/eps V and LgV in closed form.

The QP data (P, c, A, b, G, h) come from oracle.ll_build_qp, whose assembly tests/test_ll_oracle.py
pins against closed forms.
"""
import numpy as np

LD = np.longdouble
# the reference needs an extended-precision longdouble; the test modules built on it skip with this reason where
# it is none (epilogue_np and clf_np are plain fp64 and stay usable), and ipm_ld refuses to run
EXTENDED = bool(np.finfo(LD).eps < 1e-18)
NOT_EXTENDED = "np.longdouble is not an extended-precision type here (eps %g)" % np.finfo(LD).eps

OPTIMAL, FAILED, MAXIT = 0, 1, 2


def _lu_ld(K):
    """In-place LU of K (longdouble, square) with partial pivoting: (LU, row order) or None if singular."""
    K = K.copy()
    d = K.shape[0]
    perm = np.arange(d)
    for k in range(d):
        r = k + int(np.argmax(np.abs(K[k:, k])))
        if K[r, k] == 0:
            return None
        if r != k:
            K[[k, r]] = K[[r, k]]
            perm[[k, r]] = perm[[r, k]]
        K[k + 1:, k] /= K[k, k]
        K[k + 1:, k + 1:] -= np.outer(K[k + 1:, k], K[k, k + 1:])
    return K, perm


def _lu_solve_ld(lu, rhs):
    K, perm = lu
    d = K.shape[0]
    v = rhs[perm].copy()
    for k in range(1, d):
        v[k] -= K[k, :k] @ v[:k]
    for k in range(d - 1, -1, -1):
        v[k] = (v[k] - K[k, k + 1:] @ v[k + 1:]) / K[k, k]
    return v


def _steplen(v, dv):
    """findsteplength: the largest step keeping v + a dv >= 0, 1 when nothing blocks below 1e10."""
    neg = dv < 0
    if not neg.any():
        return LD(1)
    a = (-(v[neg] / dv[neg])).min()
    return a if a < LD(1e10) else LD(1)


def ipm_ld(Pd, c, A, b, G, h, maxit=25, tol=1e-6):
    """Returns (xs, flag, iters): xs[k] is x after k iterations (xs[0] the initial point), as float64
    arrays rounded from the longdouble iterates."""
    assert EXTENDED, NOT_EXTENDED
    Pd, c, A, b, G, h = (np.asarray(v, dtype=LD) for v in (Pd, c, A, b, G, h))
    n, p, m = Pd.size, b.size, h.size
    d = n + p + m
    K = np.zeros((d, d), dtype=LD)
    K[np.arange(n), np.arange(n)] = Pd
    K[:n, n:n + p] = A.T
    K[n:n + p, :n] = A
    K[:n, n + p:] = G.T
    K[n + p:, :n] = G
    wd = np.arange(n + p, d)

    def factor(w):
        K[wd, wd] = -w
        return _lu_ld(K)

    def solve(lu, r1, r2, r3):
        v = _lu_solve_ld(lu, np.concatenate([r1, r2, r3]))
        return v[:n], v[n:n + p], v[n + p:]

    # kkt_initialize: W = I, rhs (-c, b, h)
    lu = factor(np.ones(m, dtype=LD))
    if lu is None:
        return [np.zeros(n)], FAILED, 0
    x, y, _ = solve(lu, -c, b, h)
    zi = h - G @ x
    ap, ad = -zi.min(), zi.max()
    s = zi if ap < 0 else zi + (1 + ap)
    z = -zi if ad < 0 else -zi + (1 + ad)

    xs = [np.asarray(x, dtype=np.float64)]
    th = LD(tol) / np.sqrt(LD(3))
    tol = LD(tol)
    step = LD(0.99)
    flag, it = MAXIT, 0
    for _ in range(maxit):
        rx = -Pd * x - c - G.T @ z - A.T @ y
        ry = b - A @ x
        rz = h - s - G @ x
        sz = s @ z
        if np.sqrt(rx @ rx) < th and np.sqrt(rz @ rz) < th and np.sqrt(ry @ ry) < th and sz / m < tol:
            flag = OPTIMAL
            break
        mu = sz / m
        lu = factor(s / z)
        if lu is None:
            flag = FAILED
            break
        # predictor
        ds = -s * z
        _, _, dz = solve(lu, rx, ry, rz - ds / z)
        dsv = (ds - s * dz) / z
        alp, ald = _steplen(s, dsv), _steplen(z, dz)
        rho = ((s + alp * dsv) @ (z + ald * dz)) / sz
        sigma = min(max(rho, LD(0)), LD(1)) ** 3
        # corrector
        ds = -s * z - dsv * dz + sigma * mu
        dx, dy, dz = solve(lu, rx, ry, rz - ds / z)
        dsv = (ds - s * dz) / z
        alp, ald = _steplen(s, dsv), _steplen(z, dz)
        alp = min(step * alp, LD(1))
        ald = min(step * ald, LD(1))
        x = x + alp * dx
        s = s + alp * dsv
        y = y + ald * dy
        z = z + ald * dz
        it += 1
        xs.append(np.asarray(x, dtype=np.float64))
    return xs, flag, it


def mat(batch, key, a, rows, ld, cols):
    """column-major (ld) storage -> numpy matrix (rows x cols)"""
    return np.asarray(batch[key][a]).reshape(cols, ld).T[:rows, :cols]


def clf_np(kp, kd, eps, y, dy):
    """CLF scalars of LowLevelCtrl::constraints in closed form, PP = [[P1/e^2, Pd/e], [Pd/e, P2]] (x) I and
    eta = [y; dy]: (V, LfV, cc/eps V, LgV)."""
    P1 = (kd * kd + kp * kp + kp) / (2 * kp * kd); Pdd = 1 / (2 * kp); P2 = (kp + 1) / (2 * kd * kp)
    cc = 1 / (0.5 * (P1 + P2 + np.sqrt((P1 - P2) ** 2 + 4 * Pdd ** 2)))
    V = np.sum(P1 / eps ** 2 * y * y + 2 * Pdd / eps * y * dy + P2 * dy * dy)
    v2 = -kp * y - kd * dy
    LfV = 2 * np.sum((P1 / eps ** 2 * y + Pdd / eps * dy) * dy + (Pdd / eps * y + P2 * dy) * v2)
    LgV = 2 * (Pdd / eps * y + P2 * dy)
    return V, LfV, cc / eps * V, LgV


def epilogue_np(batch, a, x):
    """calcTorque after the QP (LowLevelCtrl.cpp:44-98, swingInvKin :446-488) for agent a from the QP
    solution x: dict of QP_force, tau, ddq, dq, q."""
    g = batch
    ind = g["ind"][a]
    c_ = int((ind == 1).sum())
    con, sw = 3 * c_, 12 - 3 * c_
    Dinv = mat(g, "Dinv", a, 18, 18, 18)
    B = mat(g, "B", a, 18, 18, 12)
    Jtoe = mat(g, "Jtoe", a, 12, 12, 18)
    Jhip = mat(g, "Jhip", a, 12, 12, 18)
    Js = mat(g, "Js", a, sw, 12, 18)
    toe = g["toePos"][a].reshape(4, 3); hip = g["hipPos"][a].reshape(4, 3)
    q, dq, hd, dhd = g["q"][a], g["dq"][a], g["hd"][a], g["dhd"][a]
    F = np.zeros(12); k = 0
    for i in range(4):
        if ind[i] == 1:
            F[3 * i:3 * i + 3] = x[k:k + 3]; k += 3
    tau = np.array(g["tau"][a], float)
    tau[6:] = x[con:con + 12]
    if sw:
        Delta = np.linalg.inv(Js @ Dinv @ Js.T)
        pd = np.zeros(sw); vd = np.zeros(sw); cs = 0
        for i in range(4):
            if ind[i] == 0:
                pd[cs:cs + 3] = hd[6 + cs:9 + cs] - toe[i]
                vd[cs:cs + 3] = dhd[6 + cs:9 + cs] - Jtoe[3 * i:3 * i + 3] @ dq
                cs += 3
        tau += Js.T @ (1600 * np.diag(Delta) * pd + 40 * vd)
    ddq = Dinv @ (B @ tau[6:] + Jtoe.T @ F - g["Hv"][a])
    dqn = dq + ddq / 1000
    qn = q + dqn / 1000 + 0.5e-6 * ddq
    cs = 0
    for i in range(4):
        if ind[i] == 0:
            Jt = Jtoe[3 * i:3 * i + 3] - Jhip[3 * i:3 * i + 3]
            r = (dhd[6 + cs:9 + cs] - Jhip[cs:cs + 3] @ dq) + 20 * ((hd[6 + cs:9 + cs] - hip[i]) - (toe[i] - hip[i])) \
                - Jt[:, 3:6] @ dq[3:6]
            v = np.linalg.solve(Jt[:, 6 + 3 * i:9 + 3 * i], r)
            dqn[6 + 3 * i:9 + 3 * i] = v
            qn[6 + 3 * i:9 + 3 * i] = q[6 + 3 * i:9 + 3 * i] + v / 1000
            cs += 3
    return dict(QP_force=F, tau=tau, ddq=ddq, dq=dqn, q=qn)
