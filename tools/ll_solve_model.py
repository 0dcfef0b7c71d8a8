"""CPU, numpy fp64: a model of the Newton solve of the low-level CLF-QP kernel (csrc/srb_llctrl.hip), run through
the iSWIFT iteration on the stress cases of tests/ll_cases.py and judged against the extended-precision reference
(tests/ll_reference.py).  It is how the MAXIT stalls at active bounds were traced to the way dx was formed
(DESIGN.md 6b); it needs no GPU.

    python tools/ll_solve_model.py [--residual] [case ...]

The model keeps the kernel's structure: H = P + G' Omega G solved block by block (the friction LDL' of each stance
leg by substitution, diagonal torques, Sherman-Morrison aux / defect block with the CLF row's r3 kept out of
omega r3), Y = H^-1 A', S = A Y inverted by Gauss-Jordan without pivoting, dz = Omega (G dx - r3).  Variants:
    separate   dx = H^-1 g - Y dy, two block solves rounded separately (the kernel before the fix)
    combined   dx = H^-1 (r1 - A' dy + G' Omega r3), one block solve of the combined right-hand side
    refined    combined + iterative refinement on the unreduced system: at least one step, at most REFINE, while a
               correction exceeds REFINE_TOL of its part of the step (the kernel now)
Per case and variant: agents at MAXIT, agents whose (status, iters) is neither the reference's nor the oracle's, the
worst trajectory error against the bound of tests/test_ll_gpu_stress.py, mean refinement steps per solve.
--residual: for the combined solve, the quantiles of the unreduced residual (max norm over the largest term) of the
solves whose first correction is above and below 1e-9 of the step -- they overlap down to machine epsilon, which is
why the first refinement step is not made conditional on the residual.
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "srb-cbf-nmpc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle  # noqa: E402
import ll_cases  # noqa: E402

REFINE, REFINE_TOL = 3, 1e-6      # SRB_LL_REFINE, SRB_LL_REFINE_TOL (csrc/srb_kernel_params.h)


def _amax(v):
    return np.abs(v).max() if v.size else 0.0


def _gj_inv(S):
    n = S.shape[0]
    M = np.hstack([S.copy(), np.eye(n)])
    for k in range(n):
        M[k] /= M[k, k]
        for i in range(n):
            if i != k:
                M[i] -= M[i, k] * M[k]
    return M[:, n:]


class Solve:
    def __init__(self, Pd, A, G, variant):
        self.Pd, self.A, self.G, self.variant = Pd, A, G, variant
        n, m = Pd.size, G.shape[0]
        self.clf = 1 if (n - 12) % 3 == 1 else 0
        self.cnt = (m - 24 - self.clf) // 5
        self.con, self.nft = 3 * self.cnt, 3 * self.cnt + 12
        self.steps = self.solves = 0
        self.residual = []             # (eta, first correction) per solve

    def factor(self, w):
        s = self
        s.w, s.om = w, 1.0 / w
        s.L = []
        for l in range(s.cnt):
            w0, w1, w2, w3, w4 = s.om[5 * l:5 * l + 5]
            d, mu = s.Pd[3 * l], -s.G[5 * l, 3 * l + 2]
            a, b = d + w0 + w1, d + w2 + w3
            sig = d + w4 + mu * mu * (d * (w0 + w1) + 4.0 * w0 * w1) / a + mu * mu * (d * (w2 + w3) + 4.0 * w2 * w3) / b
            s.L.append((a, b, sig, -mu * (w1 - w0) / a, -mu * (w3 - w2) / b))
        c5 = 5 * s.cnt
        s.hinv = 1 / (s.Pd[s.con:s.nft] + s.om[c5:c5 + 12] + s.om[c5 + 12:c5 + 24])
        s.Dd = s.Pd[s.nft:]
        if s.clf:
            s.u = s.G[-1, s.nft:]
            s.v = s.u / s.Dd
            s.gam = 1 / (w[-1] + s.u @ s.v)
        z3 = np.zeros(s.G.shape[0])
        s.Y = np.stack([s.hsolve(s.A[k], z3) for k in range(s.A.shape[0])], 1)
        s.Si = _gj_inv(s.A @ s.Y)

    def hsolve(self, r1, r3):
        """H^-1 (r1 + G' Omega r3)"""
        s = self
        rows = 5 * s.cnt + 24
        g = r1.copy()
        g[:s.nft] += s.G[:rows, :s.nft].T @ (s.om[:rows] * r3[:rows])
        out = np.zeros(s.Pd.size)
        for l, (a, b, sig, l0, l1) in enumerate(s.L):
            g0, g1, g2 = g[3 * l:3 * l + 3]
            u2 = (g2 + l0 * g0 + l1 * g1) / sig
            out[3 * l:3 * l + 3] = [g0 / a + l0 * u2, g1 / b + l1 * u2, u2]
        out[s.con:s.nft] = g[s.con:s.nft] * s.hinv
        ra = r1[s.nft:]
        out[s.nft:] = ra / s.Dd
        if s.clf:
            out[s.nft:] += s.gam * s.v * (r3[-1] - s.v @ ra)
        return out

    def solve1(self, r1, r2, r3):
        s = self
        u = s.hsolve(r1, r3)
        dy = s.Si @ (s.A @ u - r2)
        dx = u - s.Y @ dy if s.variant == "separate" else s.hsolve(r1 - s.A.T @ dy, r3)
        return dx, dy, s.om * (s.G @ dx - r3)

    def solve(self, r1, r2, r3):
        s = self
        dx, dy, dz = s.solve1(r1, r2, r3)
        s.solves += 1
        for q in range(REFINE if s.variant in ("refined", "residual") else 0):
            t1 = (s.Pd * dx, s.A.T @ dy, s.G.T @ dz)
            Ax, Gx, wz = s.A @ dx, s.G @ dx, s.w * dz
            e1, e2, e3 = r1 - sum(t1), r2 - Ax, r3 - (Gx - wz)
            ex, ey, ez = s.solve1(e1, e2, e3)
            if s.variant == "residual":      # record only: the step stays the combined one
                scale = max(max(map(_amax, t1)), _amax(r1), _amax(Ax), _amax(r2), _amax(Gx), _amax(wz), _amax(r3), 1e-300)
                s.residual.append((max(_amax(e1), _amax(e2), _amax(e3)) / scale,
                                   max(_amax(ex) / max(_amax(dx), 1e-300), _amax(ez) / max(_amax(dz), 1e-300))))
                break
            dx, dy, dz = dx + ex, dy + ey, dz + ez
            s.steps += 1
            if not (_amax(ex) > REFINE_TOL * _amax(dx) or _amax(ey) > REFINE_TOL * _amax(dy)
                    or _amax(ez) > REFINE_TOL * _amax(dz)):
                break
        return dx, dy, dz


def _steplen(v, dv):
    neg = dv < 0
    if not neg.any():
        return 1.0
    a = (-(v[neg] / dv[neg])).min()
    return a if a < 1e10 else 1.0


def ipm(Pd, c, A, b, G, h, maxit, tol, K):
    """the iteration of tests/ll_reference.py ipm_ld in fp64 with K's Newton solves: (x iterates, flag, iters)"""
    m = h.size
    K.factor(np.ones(m))
    x, y, _ = K.solve(-c, b, h)
    zi = h - G @ x
    ap, ad = -zi.min(), zi.max()
    s = zi if ap < 0 else zi + (1 + ap)
    z = -zi if ad < 0 else -zi + (1 + ad)
    xs, th, flag, it = [x.copy()], tol / np.sqrt(3.0), 2, 0
    for _ in range(maxit):
        rx = -Pd * x - c - G.T @ z - A.T @ y
        ry = b - A @ x
        rz = h - s - G @ x
        sz = s @ z
        if np.linalg.norm(rx) < th and np.linalg.norm(rz) < th and np.linalg.norm(ry) < th and sz / m < tol:
            flag = 0
            break
        K.factor(s / z)
        ds = -s * z
        _, _, dz = K.solve(rx, ry, rz - ds / z)
        dsv = (ds - s * dz) / z
        alp, ald = _steplen(s, dsv), _steplen(z, dz)
        sigma = min(max(((s + alp * dsv) @ (z + ald * dz)) / sz, 0.0), 1.0) ** 3
        ds = -s * z - dsv * dz + sigma * sz / m
        dx, dy, dz = K.solve(rx, ry, rz - ds / z)
        dsv = (ds - s * dz) / z
        alp, ald = min(0.99 * _steplen(s, dsv), 1.0), min(0.99 * _steplen(z, dz), 1.0)
        x, s, y, z = x + alp * dx, s + alp * dsv, y + ald * dy, z + ald * dz
        it += 1
        xs.append(x.copy())
    return xs, flag, it


def run_case(name, variant):
    t = ll_cases.trajectories(name)
    p = oracle.ll_params(**t["params"])
    stalls = neither = steps = solves = 0
    worst, residual = 0.0, []
    for a in range(ll_cases.A):
        Pd, c, A, b, G, h, *_ = oracle.ll_build_qp(p, t["batch"], a)
        K = Solve(Pd, A, G, variant)
        with np.errstate(all="ignore"):
            xs, f, it = ipm(Pd, c, A, b, G, h, t["maxit"], p.tol, K)
        stalls += f == 2
        neither += (f, it) not in ((t["ref_flag"][a], t["ref_it"][a]), (t["orc_flag"][a], t["orc_it"][a]))
        for k in range(min(it, t["ref_it"][a], t["orc_it"][a]) + 1):
            worst = max(worst, float(ll_cases.rel_err(np.pad(xs[k], (0, 32 - xs[k].size)), t["ref_x"][a][k])))
        steps, solves = steps + K.steps, solves + K.solves
        residual += K.residual
    return stalls, neither, worst, max(1e-8, 10 * t["E_orc"]), steps / solves, residual


def main():
    args = sys.argv[1:]
    residual = args[:1] == ["--residual"]
    names = args[residual:] or list(ll_cases.CASES)
    if residual:
        print("unreduced residual / largest term after the combined solve, quantiles 0 10 50 90 100 %, by the size of")
        print("the first correction (max of |ex|/|dx|, |ez|/|dz|)")
        for n in names:
            r = np.array(run_case(n, "residual")[5])
            r = r[np.isfinite(r).all(1)]
            big = r[:, 1] > 1e-9
            for lab, msk in (("> 1e-9", big), ("<= 1e-9", ~big)):
                q = np.quantile(r[msk, 0], [0, .1, .5, .9, 1]) if msk.any() else []
                print(f"{n:<13} correction {lab:<8} {int(msk.sum()):4d} solves  " + " ".join(f"{v:.1e}" for v in q), flush=True)
        return
    print(f"{'case':<13}{'variant':<10}{'@MAXIT':>7}{'neither':>8}{'traj err':>10}{'bound':>10}{'':>6}{'steps/solve':>12}")
    for n in names:
        for v in ("separate", "combined", "refined"):
            st, ne, w, B, sp, _ = run_case(n, v)
            print(f"{n:<13}{v:<10}{st:>7}{ne:>8}{w:>10.1e}{B:>10.1e}{'ok' if w <= B else 'OVER':>6}{sp:>12.2f}", flush=True)


if __name__ == "__main__":
    main()
