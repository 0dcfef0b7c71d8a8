/*
 * ORACLE (test infrastructure only): NLP stage.
 *
 * The reference solves (MPC_dist.cpp:402-427, dec_vars_constr_cost.h:148-438)
 *     min 0.5 x'Q_qp x + f'x   s.t.  Aeq x = beq,  Gineq x <= hineq,
 *         (x_k - o_x)^2 + (y_k - o_y)^2 + s >= 1.9f     (obstacle "CBF" rows, :262-265)
 *         -0.35f <= xdot_k, ydot_k <= 0.35f            (velocity rows, :270-279)
 * with SNOPT 7.7.7 warm-started from the QP solution (ExVariables, :99).  SNOPT is
 * proprietary and not vendored, so this stage is OUR algorithm: a Mehrotra
 * predictor-corrector primal-dual interior-point method on the same rows, with the
 * exact Lagrangian Hessian  Q_qp - 2 sum_j z_kj I(x_k, y_k)  and inertia correction
 * Hl + delta*I whenever the reduced Hessian on null(Aeq) is not positive definite.
 * The GPU kernel implements the same iteration in condensed (null-space) form; this
 * oracle solves the full-space system [Hl + J'W^-1 J, A'; A, 0] by LU so that the two
 * share no linear-algebra code.  Independent pin: KKT certificate + SciPy (tests/).
 *
 * Row order (mirrors NeqConstraints::GetValues): [Gineq rows | obstacle rows k-major
 * (k*K + j) | velocity rows +xdot_k, +ydot_k, -xdot_k, -ydot_k].  Two-sided velocity
 * bounds become two one-sided rows.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include "oracle.h"

/* initial inequality duals: 100, the scale of the tracking weights' multipliers (against 1:
 * 20-25 % fewer NLP iterations on the bench/test workloads, profiles/r01_nlp_z0_scan.txt) */
#define ORC_NLP_Z0 100.0
/* a step shorter than this from a near-optimal iterate ends the NLP as ACCEPTABLE (4) */
#define ORC_NLP_BLOCKED 0.05
/* OPTIMAL also needs the last primal step max|ap dx| below this: the residual tests alone
 * (dual residual scaled by max(1, |Q x + f|_inf)) left 73 of 2048 N = 20 solves 1e-4..5e-4
 * from the optimum along flat directions; with the step test every one is within 2.1e-5
 * (profiles/r02_nlp_exit.txt) */
/* round 3: with the active-set polish after every solve (below), the interior-point iteration
 * only has to identify the active set: the dual-residual and complementarity tests are 10x looser
 * (ORC_NLP_EXITF) and the last-step test is off (ORC_NLP_DXTOL).  On the bench batches the NLP
 * takes 15 % fewer iterations (configs[2]: 8.14 -> 6.85 on average, 12 -> 10 at most) and every
 * polished result is unchanged within 4e-7 (the kernel: SRB_NLP_EXITF / SRB_NLP_DXTOL). */
#define ORC_NLP_EXITF 10.0
#define ORC_NLP_DXTOL 1e300
/* ... and after this many near-optimal iterates (primal and complementarity tests met, dual
 * residual within 100x of its threshold) without meeting both, the solve is at its round-off
 * floor: ACCEPTABLE (4) at the current iterate */
#define ORC_NLP_NEARWAIT 4

typedef struct {
    int n, p, mq, K, N, mo, mv, m;
    const double *Pd, *c, *A, *b, *G, *h, *obs, *eps;
    int *gnz; double *gval;
} nlp_t;

static void rows_eval(const nlp_t *P, const double *x, double *g, double *Jv /* [m][4] */, int *Ji /* [m][4] */)
{
    const int n = P->n;
    for (int r = 0; r < P->mq; r++) {
        double s = 0;
        for (int k = 0; k < 4; k++) {
            int j = P->gnz[4 * r + k];
            Ji[4 * r + k] = j; Jv[4 * r + k] = P->gval[4 * r + k];
            if (j >= 0) s += P->gval[4 * r + k] * x[j];
        }
        g[r] = s;
    }
    int r = P->mq;
    for (int k = 0; k < P->N; k++)
        for (int j = 0; j < P->K; j++, r++) {
            double dx = x[4 * k] - P->obs[(k * P->K + j) * 2];
            double dy = x[4 * k + 2] - P->obs[(k * P->K + j) * 2 + 1];
            g[r] = -(dx * dx + dy * dy) - x[n - 1];
            Ji[4 * r + 0] = 4 * k;     Jv[4 * r + 0] = -2 * dx;
            Ji[4 * r + 1] = 4 * k + 2; Jv[4 * r + 1] = -2 * dy;
            Ji[4 * r + 2] = n - 1;     Jv[4 * r + 2] = -1.0;
            Ji[4 * r + 3] = -1;        Jv[4 * r + 3] = 0.0;
        }
    for (int sg = 1; sg >= -1; sg -= 2)
        for (int comp = 1; comp <= 3; comp += 2)
            for (int k = 0; k < P->N; k++, r++) {
                g[r] = sg * x[4 * k + comp];
                Ji[4 * r] = 4 * k + comp; Jv[4 * r] = sg;
                for (int t = 1; t < 4; t++) { Ji[4 * r + t] = -1; Jv[4 * r + t] = 0; }
            }
}

static double dotv(const double *a, const double *b, int n) { double s = 0; for (int i = 0; i < n; i++) s += a[i] * b[i]; return s; }
static double steplen(const double *v, const double *dv, int m)
{
    double a = 1e10; int f = 0;
    for (int i = 0; i < m; i++)
        if (dv[i] < 0 && (-v[i] / dv[i]) < a) { a = -(v[i] / dv[i]); f = 1; }
    return f ? a : 1.0;
}

/* null-space basis of Aeq by forward rollout (used only for the PD test) */
static void build_Z(const orc_params *pp, const double *foot, double *Z, int n, int nz)
{
    const int N = pp->N, C = pp->C;
    double Ad[16], Bd[8];
    orc_lip(pp, Ad, Bd);
    memset(Z, 0, sizeof(double) * (size_t)n * nz);
    for (int j = 0; j < N; j++)
        for (int t = 0; t < C - 1; t++) {
            int col = j * (C - 1) + t;
            double lam[4] = {0, 0, 0, 0}, gg[2] = {0, 0}, v[4], tt[4];
            int is_null = 0;
            const double *F = foot + (size_t)j * 2 * C;
            if (C != 4) { lam[t] = 1.0; lam[C - 1] = -1.0; }
            else {  /* exact null vector of [F; 1'] replaces one column (see the GPU kernel) */
                double nv4[4];
                for (int i = 0; i < 4; i++) {
                    int ci[3], q = 0;
                    for (int k = 0; k < 4; k++) if (k != i) ci[q++] = k;
                    double det = F[ci[0]] * (F[4 + ci[1]] - F[4 + ci[2]]) - F[ci[1]] * (F[4 + ci[0]] - F[4 + ci[2]]) +
                                 F[ci[2]] * (F[4 + ci[0]] - F[4 + ci[1]]);
                    nv4[i] = (i & 1) ? -det : det;
                }
                int is = 0;
                for (int i = 1; i < 3; i++) if (fabs(nv4[i]) > fabs(nv4[is])) is = i;
                if (t == 2) { for (int i = 0; i < 4; i++) lam[i] = nv4[i] / nv4[is]; is_null = 1; }
                else { int i = (t < is) ? t : t + 1; lam[i] = 1.0; lam[3] = -1.0; }
            }
            if (!is_null)
                for (int i = 0; i < C; i++) { gg[0] += F[i] * lam[i]; gg[1] += F[C + i] * lam[i]; }
            for (int i = 0; i < C; i++) Z[(size_t)(6 * N + C * j + i) * nz + col] = lam[i];
            Z[(size_t)(4 * N + 2 * j) * nz + col] = gg[0];
            Z[(size_t)(4 * N + 2 * j + 1) * nz + col] = gg[1];
            for (int d = 0; d < 4; d++) v[d] = Bd[d * 2] * gg[0] + Bd[d * 2 + 1] * gg[1];
            for (int k = j; k < N; k++) {
                for (int d = 0; d < 4; d++) Z[(size_t)(4 * k + d) * nz + col] = v[d];
                for (int d = 0; d < 4; d++) tt[d] = Ad[d * 4] * v[0] + Ad[d * 4 + 1] * v[1] + Ad[d * 4 + 2] * v[2] + Ad[d * 4 + 3] * v[3];
                memcpy(v, tt, sizeof v);
            }
        }
    Z[(size_t)(n - 1) * nz + nz - 1] = 1.0;
}

/*
 * Active-set polish at the end of the NLP (the kernel's `polish`, srb_kernels.hip, the same
 * rules).  Near its round-off floor the barrier system's active rows carry z/s ~ 1e14, so the
 * interior-point iterate stops up to ~1e-4 from the optimum along soft directions.  From the
 * final iterate, rows with s < z are taken as the active set A and the equality-constrained
 * problem  min f(x) s.t. Aeq x = beq, g_A(x) = h_A  is solved by Newton steps on its KKT system
 * regularised by 1/rho on the constraint block,
 *     [H_L + rho J_A'J_A, Aeq'; Aeq, 0] dx = -(grad f + J_A'(z_A + rho c_A)),  z_A += rho (c_A + J_A dx),
 * (H_L = Q_qp - 2 sum z_A on the obstacle positions), whose fixed point is the exact KKT point
 * for that active set (c_A = 0).  The result replaces the iterate only if it is primal feasible
 * (every row within ORC_POLISH_PTOL of its bound), dual feasible (z_A >= 0), the Newton
 * iteration has converged, the equality rows hold to ORC_POLISH_EQTOL and the reduced stationarity Z'(grad f + J_A' z_A) is at round-off
 * level; the solve then ends OPTIMAL.  Otherwise the interior-point result stands.
 */
#define ORC_POLISH_RHO 1e9
#define ORC_POLISH_IT 5           /* at most this many Newton steps per active-set pass */
#define ORC_POLISH_PASSES 4       /* active-set passes (the most negative z_A leaves, violated rows join) */
#define ORC_POLISH_PTOL 1e-9      /* primal: g_i(x) - h_i <= this on every row, |c_A| <= this on active rows */
#define ORC_POLISH_DXTOL 1e-7     /* the last Newton correction |dx|_inf <= this (converged) */
#define ORC_POLISH_EQTOL 1e-8     /* the equality rows hold to this at an accepted point (kernel SRB_POLISH_EQTOL) */
#define ORC_POLISH_STOL 1e-6      /* ... and the Newton correction the reduced stationarity residual g = Z'(grad f + J_A' z_A)
                                     implies, |M^-1 g|_inf with M the last step's reduced matrix, is <= this (kernel
                                     SRB_POLISH_STOL): the distance to the stationary point, whatever the gradient's
                                     scale -- a guard against a point that is feasible but not stationary;
                                     round 6: at most 6e-8 on the accepted polishes of six bench workloads */
#define ORC_POLISH_OMCAP 1e-2     /* inactive rows: Hessian weight min(z/s, this), a proximal term */
#define ORC_POLISH_DX1 1e-4       /* a Newton step this small whose active rows then hold to CTOL ends the pass */
#define ORC_POLISH_CTOL 1e-10

/* The polish and exit constants below are read from the environment only in a diagnostics build of the
 * oracle (-DORC_DIAG_ENV): the library the tests load computes the same results whatever the
 * environment holds (tests/test_oracle.py test_oracle_environment_does_not_change_the_numerics). */
static double g_polish_rho = ORC_POLISH_RHO;
static double g_polish_kappa = 1e4;
static int g_polish_zinit = 1;    /* exploration: 1 = a later pass starts from the previous pass's z_A */
int orc_early_stats[2];          /* exploration counters: early polish attempts failed / accepted */
unsigned long long orc_polish_stat_max[2];   /* exploration: the largest reduced stationarity / scale of an accepted (0) /
                                                rejected (1) pass, as the bits of a non-negative double (ordered as the values) */
int orc_polish_stats[16];        /* exploration counters: [0] rejected, [1 + p] accepted after pass p */
__thread double *orc_stats_sink; /* the agent's statistics row (oracle.h ORC_NSTAT), NULL: not recorded */
static int g_polish_it = ORC_POLISH_IT, g_polish_passes = ORC_POLISH_PASSES;
static double g_polish_omcap = ORC_POLISH_OMCAP;

/* Newton steps of the regularised equality-constrained KKT for the active set `act`; returns 0
 * on success, -1 when the reduced matrix is not positive definite, -2 when the full-space LU fails */
static int polish_newton(const nlp_t *P, const double *hh, const double *Z, int nz, const int *act, const double *om,
                         double *xt, double *za, double *g, double *Jv, int *Ji, double *Hl, double *K, double *rhs,
                         double *cA, double *Hr, double *HZ, int *piv, double *lastdx, int trace)
{
    const int n = P->n, p = P->p, m = P->m, dim = n + p;
    const double rho = g_polish_rho;
    for (int it = 0; it < g_polish_it; it++) {
        rows_eval(P, xt, g, Jv, Ji);
        double cmax = 0.0;
        for (int r = 0; r < m; r++) { cA[r] = act[r] ? g[r] - hh[r] : 0.0; cmax = fmax(cmax, fabs(cA[r])); }
        /* converged after a small Newton step: its quadratic remainder on the active rows is below
         * CTOL (the kernel's SRB_POLISH_DX1 / SRB_POLISH_CTOL; saves the verifying step) */
        if (it > 0 && *lastdx <= ORC_POLISH_DX1 && cmax <= ORC_POLISH_CTOL) { *lastdx = 0.0; break; }
        memset(Hl, 0, sizeof(double) * n * n);
        for (int j = 0; j < n; j++) { Hl[j * n + j] = P->Pd[j]; rhs[j] = -(P->Pd[j] * xt[j] + P->c[j]); }
        for (int k = 0; k < P->N; k++) {
            double zs = 0;
            for (int j = 0; j < P->K; j++) zs += za[P->mq + k * P->K + j];
            Hl[(4 * k) * n + 4 * k] -= 2 * zs; Hl[(4 * k + 2) * n + 4 * k + 2] -= 2 * zs;
        }
        for (int r = 0; r < m; r++) {
            /* active rows: rho; inactive ones keep their interior-point weight z/s, capped at
             * OMCAP (om), in the Hessian only -- a proximal term that leaves the fixed point alone
             * and keeps the reduced matrix definite along directions no active row pins (lambda
             * with 4 contacts); the cap keeps it from slowing the Newton steps elsewhere */
            const double wr = act[r] ? rho : om[r];
            for (int a = 0; a < 4; a++) {
                const int ia = Ji[4 * r + a]; if (ia < 0) continue;
                if (act[r]) rhs[ia] -= Jv[4 * r + a] * (za[r] + rho * cA[r]);
                for (int bb = 0; bb < 4; bb++) { const int ib = Ji[4 * r + bb]; if (ib >= 0) Hl[ia * n + ib] += wr * Jv[4 * r + a] * Jv[4 * r + bb]; }
            }
        }
        /* the reduced matrix Z'(H_L + rho J_A'J_A)Z must be positive definite */
        for (int i = 0; i < n; i++)
            for (int a = 0; a < nz; a++) {
                double acc = 0;
                for (int j = 0; j < n; j++) acc += Hl[i * n + j] * Z[(size_t)j * nz + a];
                HZ[(size_t)i * nz + a] = acc;
            }
        for (int a = 0; a < nz; a++)
            for (int bb = 0; bb < nz; bb++) {
                double acc = 0;
                for (int i = 0; i < n; i++) acc += Z[(size_t)i * nz + a] * HZ[(size_t)i * nz + bb];
                Hr[a * nz + bb] = acc;
            }
        if (orc_chol(nz, Hr)) return -1;
        memset(K, 0, sizeof(double) * dim * dim);
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) K[i * dim + j] = Hl[i * n + j];
        for (int k = 0; k < p; k++) {
            for (int j = 0; j < n; j++) { K[(n + k) * dim + j] = P->A[(size_t)k * n + j]; K[j * dim + n + k] = P->A[(size_t)k * n + j]; }
            rhs[n + k] = P->b[k] - dotv(P->A + (size_t)k * n, xt, n);
        }
        if (orc_lu(dim, K, piv)) return -2;
        orc_lu_solve(dim, K, piv, rhs);
        double mdx = 0.0;
        for (int r = 0; r < m; r++) {
            if (!act[r]) continue;
            double jd = 0;
            for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) jd += Jv[4 * r + t] * rhs[Ji[4 * r + t]];
            za[r] += rho * (cA[r] + jd);
        }
        for (int j = 0; j < n; j++) { xt[j] += rhs[j]; mdx = fmax(mdx, fabs(rhs[j])); }
        *lastdx = mdx;
        __atomic_add_fetch(&orc_polish_stats[15], 1, __ATOMIC_RELAXED);
        if (trace) fprintf(stderr, "  polish it %d: |dx| %.3e\n", it, mdx);
        if (mdx <= ORC_POLISH_DXTOL) break;            /* converged: no further step */
    }
    return 0;
}

/* returns 1 when the polished point is accepted (x, z replaced) */
static int polish(const nlp_t *P, const double *hh, const double *Z, int nz, double *x, const double *s,
                  double *z, int trace)
{
    const int n = P->n, m = P->m, dim = n + P->p;
    double *xt = malloc(sizeof(double) * n), *za = malloc(sizeof(double) * m), *g = malloc(sizeof(double) * m);
    double *Jv = malloc(sizeof(double) * 4 * m), *Hl = malloc(sizeof(double) * n * n), *K = malloc(sizeof(double) * dim * dim);
    double *rhs = malloc(sizeof(double) * dim), *cA = malloc(sizeof(double) * m), *v = malloc(sizeof(double) * n);
    double *Hr = malloc(sizeof(double) * nz * nz), *HZ = malloc(sizeof(double) * (size_t)n * nz), *gr = malloc(sizeof(double) * nz);
    int *Ji = malloc(sizeof(int) * 4 * m), *piv = malloc(sizeof(int) * dim), *act = malloc(sizeof(int) * m);
    double *om = malloc(sizeof(double) * m);
    int ok = 0;
    for (int r = 0; r < m; r++) { act[r] = s[r] * g_polish_kappa < z[r]; za[r] = act[r] ? z[r] : 0.0; om[r] = act[r] ? 0.0 : fmin(z[r] / s[r], g_polish_omcap); }
    int npass = 0;
    for (int pass = 0; pass < g_polish_passes && !ok; pass++, npass++) {
        memcpy(xt, x, sizeof(double) * n);
        double lastdx = 1e300;
        const int pn = polish_newton(P, hh, Z, nz, act, om, xt, za, g, Jv, Ji, Hl, K, rhs, cA, Hr, HZ, piv, &lastdx, trace);
        if (pn) {
            if (pn == -1 && orc_stats_sink) orc_stats_sink[ORC_ST_POLISH_NPD] = 1.0;
            if (trace) fprintf(stderr, "  polish pass %d: reduced matrix not positive definite -> rejected\n", pass);
            break;
        }
        rows_eval(P, xt, g, Jv, Ji);
        double zm = 1.0, pv = -1e300, cv = 0.0, zmin = 1e300;
        int nact = 0, changed = 0;
        for (int r = 0; r < m; r++) {
            pv = fmax(pv, g[r] - hh[r]);
            if (act[r]) { nact++; zm = fmax(zm, fabs(za[r])); zmin = fmin(zmin, za[r]); cv = fmax(cv, fabs(g[r] - hh[r])); }
        }
        /* reduced stationarity: gradient part and multiplier part separately for the scale */
        double gf = 0.0, gz = 0.0, res = 0.0, gmax = 0.0;
        for (int j = 0; j < n; j++) { v[j] = P->Pd[j] * xt[j] + P->c[j]; gmax = fmax(gmax, fabs(v[j])); }
        for (int a = 0; a < nz; a++) { double acc = 0; for (int j = 0; j < n; j++) acc += Z[(size_t)j * nz + a] * v[j]; gr[a] = acc; gf = fmax(gf, fabs(acc)); }
        for (int j = 0; j < n; j++) v[j] = 0.0;
        for (int r = 0; r < m; r++) if (act[r]) for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) v[Ji[4 * r + t]] += Jv[4 * r + t] * za[r];
        for (int a = 0; a < nz; a++) {
            double acc = 0; for (int j = 0; j < n; j++) acc += Z[(size_t)j * nz + a] * v[j];
            gz = fmax(gz, fabs(acc)); res = fmax(res, fabs(gr[a] + acc));
            gr[a] += acc;
        }
        /* the Newton correction that residual implies, with the last step's factor (Hr: Cholesky of the reduced
         * matrix; the kernel uses its inverse of the same matrix) */
        orc_chol_solve(nz, Hr, gr);
        double sdx = 0.0;
        for (int a = 0; a < nz; a++) sdx = fmax(sdx, fabs(gr[a]));
        /* ... and the multipliers that step leaves, z_A + rho (c_A + J_A Z dxi) with dxi = -M^-1 g, keep their sign
         * (kernel polish_stationary: the same test) */
        for (int j = 0; j < n; j++) { double acc = 0; for (int a = 0; a < nz; a++) acc += Z[(size_t)j * nz + a] * gr[a]; v[j] = -acc; }
        double zn_min = 1e300, zn_max = 1.0;
        for (int r = 0; r < m; r++) {
            if (!act[r]) continue;
            double jd = 0;
            for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) jd += Jv[4 * r + t] * v[Ji[4 * r + t]];
            const double zn = za[r] + g_polish_rho * ((g[r] - hh[r]) + jd);
            zn_min = fmin(zn_min, zn); zn_max = fmax(zn_max, fabs(zn));
        }
        /* (rho |c_A| <= rho PTOL = 1 is the resolution of that update: the tolerance) */
        if (!(zn_min >= -(g_polish_rho * ORC_POLISH_PTOL + 1e-9 * zn_max))) sdx = 1e300;
        const int dual_ok = nact == 0 || zmin >= -1e-9 * zm;
        /* the equality rows (LIP dynamics, CoP, sum lambda; dec_vars_constr_cost.h:154-206) at the
         * polished point: the kernel's SRB_POLISH_EQTOL test (the LU step keeps them to round-off) */
        double eqr = 0.0;
        for (int k = 0; k < P->p; k++) eqr = fmax(eqr, fabs(dotv(P->A + (size_t)k * n, xt, n) - P->b[k]));
        /* a converged Newton iteration (the last correction) makes the reduced gradient of the Lagrangian
         * O(|H| |dx|); round 6 tests it as well, from the problem data (grad f = Pd x + c) and the polish's own
         * multipliers: a point that is feasible, converged and dual feasible but not stationary -- what the
         * round-5 generic-pointer build returned as OPTIMAL -- is rejected (kernel, same rule) */
        ok = pv <= ORC_POLISH_PTOL && cv <= ORC_POLISH_PTOL && dual_ok && lastdx <= ORC_POLISH_DXTOL && eqr <= ORC_POLISH_EQTOL &&
             sdx <= ORC_POLISH_STOL;
        if (trace)
            fprintf(stderr, "  polish pass %d: |A| %d  primal %.2e  |c_A| %.2e  zmin %.2e (zmax %.2e)  last dx %.2e  stat %.2e (scale %.2e)  -> %s\n",
                    pass, nact, pv, cv, nact ? zmin : 0.0, zm, lastdx, res, fmax(1.0, gmax), ok ? "accepted" : "rejected");
        if (trace > 1)
            for (int r = 0; r < m; r++)
                if (act[r] || g[r] - hh[r] > ORC_POLISH_PTOL)
                    fprintf(stderr, "    row %3d (%s) act %d  s %.3e z %.3e  za %.4e  g-h %.3e\n", r,
                            r < P->mq ? "lin" : r < P->mq + P->mo ? "obs" : "vel", act[r], s[r], z[r], za[r], g[r] - hh[r]);
        {
            const double sr = sdx;
            unsigned long long bits, *dst = &orc_polish_stat_max[ok ? 0 : 1], cur = __atomic_load_n(dst, __ATOMIC_RELAXED);
            memcpy(&bits, &sr, sizeof bits);
            while (bits > cur && !__atomic_compare_exchange_n(dst, &cur, bits, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
        }
        if (ok) break;
        /* next pass: the row with the most negative multiplier leaves the active set (one at a
         * time: near-dependent active rows -- one obstacle at consecutive grids -- share large
         * multipliers of both signs, and dropping all negative ones at once loses rows the
         * solution needs), violated rows join */
        int worst = -1;
        for (int r = 0; r < m; r++)
            if (act[r] && za[r] < -1e-9 * zm && (worst < 0 || za[r] < za[worst])) worst = r;
        if (worst >= 0) { act[worst] = 0; changed = 1; }
        for (int r = 0; r < m; r++)
            if (!act[r] && r != worst && g[r] - hh[r] > ORC_POLISH_PTOL) { act[r] = 1; changed = 1; }
        for (int r = 0; r < m; r++) za[r] = act[r] ? (g_polish_zinit ? fmax(za[r], 0.0) : fmax(z[r], 0.0)) : 0.0;
        if (!changed) break;
    }
    if (ok) {
        memcpy(x, xt, sizeof(double) * n);
        for (int r = 0; r < m; r++) z[r] = za[r];
    }
    __atomic_add_fetch(&orc_polish_stats[ok ? 1 + npass : 0], 1, __ATOMIC_RELAXED);
    free(xt); free(za); free(g); free(Jv); free(Hl); free(K); free(rhs); free(cA); free(v); free(Hr); free(HZ); free(gr);
    free(Ji); free(piv); free(act); free(om);
    return ok;
}

int orc_nlp_solve(const orc_params *pp, const double x0[4], const double *foot,
                  const double *Pd, const double *c, const double *A, const double *b,
                  const double *G, const double *h,
                  const double *obs, const double *eps,
                  const double *x_init, double *x_out, int *iters_out)
{
    (void)x0;
    nlp_t P;
    P.N = pp->N; P.n = orc_nv(pp); P.p = orc_neq(pp); P.mq = orc_mqp(pp);
    P.K = pp->K_obs + pp->K_nbr; P.mo = P.N * P.K; P.mv = 4 * P.N; P.m = P.mq + P.mo + P.mv;
    P.Pd = Pd; P.c = c; P.A = A; P.b = b; P.G = G; P.h = h; P.obs = obs; P.eps = eps;
    const int n = P.n, p = P.p, m = P.m, dim = n + p;
    const int nz = P.N * (pp->C - 1) + 1;
    P.gnz = malloc(sizeof(int) * 4 * P.mq); P.gval = malloc(sizeof(double) * 4 * P.mq);
    for (int r = 0; r < P.mq; r++) {
        int k = 0;
        for (int j = 0; j < 4; j++) { P.gnz[4 * r + j] = -1; P.gval[4 * r + j] = 0; }
        for (int j = 0; j < n && k < 4; j++)
            if (G[(size_t)r * n + j] != 0.0) { P.gnz[4 * r + k] = j; P.gval[4 * r + k] = G[(size_t)r * n + j]; k++; }
    }
    double *hh = malloc(sizeof(double) * m);
    for (int r = 0; r < P.mq; r++) hh[r] = h[r];
    for (int r = 0; r < P.mo; r++) hh[P.mq + r] = -eps[r % P.K];
    for (int r = 0; r < P.mv; r++) hh[P.mq + P.mo + r] = pp->vsat;

    double *x = malloc(sizeof(double) * n), *q = calloc(n, sizeof(double));
    double *s = malloc(sizeof(double) * m), *z = malloc(sizeof(double) * m);
    double *g = malloc(sizeof(double) * m), *Jv = malloc(sizeof(double) * 4 * m);
    int *Ji = malloc(sizeof(int) * 4 * m);
    double *rx = malloc(sizeof(double) * n), *ry = malloc(sizeof(double) * (p + 1)), *rz = malloc(sizeof(double) * m);
    double *lam = malloc(sizeof(double) * m), *wgt = malloc(sizeof(double) * m), *ds = malloc(sizeof(double) * m);
    double *dsv = malloc(sizeof(double) * m), *dz = malloc(sizeof(double) * m), *r3 = malloc(sizeof(double) * m);
    double *K = malloc(sizeof(double) * dim * dim), *Hl = malloc(sizeof(double) * n * n);
    double *rhs = malloc(sizeof(double) * dim), *dx = malloc(sizeof(double) * n), *dq = malloc(sizeof(double) * n);
    double *hdiag = malloc(sizeof(double) * n);
    double *Z = malloc(sizeof(double) * (size_t)n * nz), *Hr = malloc(sizeof(double) * nz * nz), *HZ = malloc(sizeof(double) * (size_t)n * nz);
    int *piv = malloc(sizeof(int) * dim);
    int flag = 2, it = 0;
    /* statistics (orc_stats_sink): the exit rule and the inertia loop's counts; they steer nothing */
    int st_exit = ORC_EXIT_MAXIT, st_shift_iters = 0, st_failed = 0, st_max_tries = 0;
    double st_max_delta = 0.0;
    build_Z(pp, foot, Z, n, nz);

    memcpy(x, x_init, sizeof(double) * n);
    rows_eval(&P, x, g, Jv, Ji);
    {   /* slacks: iSWIFT-style shift of h - g(x); duals below */
        double mn = hh[0] - g[0];
        for (int r = 1; r < m; r++) if (hh[r] - g[r] < mn) mn = hh[r] - g[r];
        double ap = -mn;
        for (int r = 0; r < m; r++) { s[r] = (ap < 0) ? hh[r] - g[r] : hh[r] - g[r] + (1 + ap); z[r] = ORC_NLP_Z0; }
        /* duals z_r = ORC_NLP_Z0 / max(s_r, 1) (round 3; the kernel's SRB_NLP_Z0, the same rule):
         * rows whose slack is far from the bound (the +-1e3 boxes) start at complementarity Z0
         * instead of z = Z0; on the bench batches the NLP needs 8.1 / 8.5 iterations on average
         * against 8.9 / 9.3 (N = 10 / 20) and at most 12 / 13 against 13 / 17.  The floor keeps
         * rows the QP left at their bound (s ~ 1e-12 when no shift is needed) from z ~ 1e14 */
        for (int r = 0; r < m; r++) z[r] = ORC_NLP_Z0 / fmax(s[r], 1.0);
    }
    {   /* q = A'y, y = argmin |A'y + (Px + c + J'z)|  ->  (A A') y = -A v */
        double *v = malloc(sizeof(double) * n), *AAt = malloc(sizeof(double) * (p ? p * p : 1)), *yy = malloc(sizeof(double) * (p + 1));
        for (int j = 0; j < n; j++) v[j] = Pd[j] * x[j] + c[j];
        for (int r = 0; r < m; r++) for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) v[Ji[4 * r + t]] += Jv[4 * r + t] * z[r];
        for (int i = 0; i < p; i++) {
            for (int j = 0; j < p; j++) AAt[i * p + j] = dotv(A + (size_t)i * n, A + (size_t)j * n, n);
            yy[i] = -dotv(A + (size_t)i * n, v, n);
        }
        orc_chol(p, AAt); orc_chol_solve(p, AAt, yy);
        for (int j = 0; j < n; j++) { double sacc = 0; for (int i = 0; i < p; i++) sacc += A[(size_t)i * n + j] * yy[i]; q[j] = sacc; }
        free(v); free(AAt); free(yy);
    }

    const double tol = pp->tol, th = tol / sqrt(3.0);
    const int trace = getenv("ORC_NLP_TRACE") ? atoi(getenv("ORC_NLP_TRACE")) + 1 : 0;   /* diagnostics on stderr (2: polish rows) */
    /* diagnostics: ORC_NLP_EXIT="fx fmu acc" scales the dual-residual threshold, the
     * complementarity threshold and the ACCEPTABLE window (exploration of exit rules only) */
    double fx = ORC_NLP_EXITF, fmu = ORC_NLP_EXITF, facc = 100.0, fdx = ORC_NLP_DXTOL;
#ifdef ORC_DIAG_ENV
    if (getenv("ORC_NLP_EXIT")) sscanf(getenv("ORC_NLP_EXIT"), "%lf %lf %lf %lf", &fx, &fmu, &facc, &fdx);
#endif
    double dxlast = 1e300;                                  /* max |ap dx| of the last update */
    int npassed = 0;                                        /* near-optimal iterates so far */
    int saved = 0, restore = 0;                             /* best near-optimal iterate */
    double best_rx = 1e300;
    int provisional = 0;
    double *xsave = malloc(sizeof(double) * n), *ssave = malloc(sizeof(double) * m), *zsave = malloc(sizeof(double) * m);
    int nearwait = ORC_NLP_NEARWAIT;
#ifdef ORC_DIAG_ENV
    if (getenv("ORC_NLP_NEARWAIT")) nearwait = atoi(getenv("ORC_NLP_NEARWAIT"));
#endif
    double tr_sigma = 0.0;
    double early_mu = 0.0, early_rz = 1e300;
    int early_tried = 0, early_done = 0;
#ifdef ORC_DIAG_ENV
    if (getenv("ORC_NLP_EARLY")) sscanf(getenv("ORC_NLP_EARLY"), "%lf %lf %lf", &early_mu, &early_rz, &fdx);
#endif
    double *xe = malloc(sizeof(double) * n), *ze = malloc(sizeof(double) * m);
    for (int iter = 0; iter < pp->nlp_maxit; iter++) {
        rows_eval(&P, x, g, Jv, Ji);
        for (int j = 0; j < n; j++) rx[j] = -(Pd[j] * x[j] + c[j]) - q[j];
        for (int r = 0; r < m; r++) for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) rx[Ji[4 * r + t]] -= Jv[4 * r + t] * z[r];
        for (int k = 0; k < p; k++) ry[k] = b[k] - dotv(A + (size_t)k * n, x, n);
        for (int r = 0; r < m; r++) rz[r] = hh[r] - s[r] - g[r];
        double nrx = sqrt(dotv(rx, rx, n)), nrz = sqrt(dotv(rz, rz, m)), nry = sqrt(dotv(ry, ry, p));
        double sz = dotv(s, z, m);
        if (!isfinite(nrx) || !isfinite(nrz) || !isfinite(sz)) { flag = 3; st_exit = ORC_EXIT_DIVERGED; break; }
        {                                          /* divergence: ORC_Z_DIV (qp_ipm.c) */
            double zm = 0.0;
            for (int r = 0; r < m; r++) zm = fmax(zm, z[r]);
            if (!(zm <= ORC_Z_DIV)) { flag = 3; st_exit = ORC_EXIT_DIVERGED; break; }
        }
        /* dual residual scaled by the objective gradient (the NLP's own criterion; the
         * QP stage keeps iSWIFT's absolute test): max(1, ||Q x + f||_inf) */
        double gmax = 1.0;
        for (int j = 0; j < n; j++) { double gj = fabs(Pd[j] * x[j] + c[j]); if (gj > gmax) gmax = gj; }
        const int pass = nrx < fx * th * gmax && nrz < th && nry < th && sz / m < fmu * tol;
        if (pass && dxlast < fdx) {
            /* the loosened tests (ORC_NLP_EXITF) rely on the polish: met only by them, the result is
             * provisional -- ACCEPTABLE unless the polish is accepted (the kernel, same rule) */
            provisional = !(nrx < th * gmax && nrz < th && nry < th && sz / m < tol);
            flag = 0; st_exit = provisional ? ORC_EXIT_PROVISIONAL : ORC_EXIT_CONVERGED; break;
        }
        /* exploration: one early polish attempt once the complementarity gap is below early_mu */
        if (early_mu > 0 && !early_tried && sz / m < early_mu && nrz < early_rz) {
            early_tried = 1;
            memcpy(xe, x, sizeof(double) * n); memcpy(ze, z, sizeof(double) * m);
            if (polish(&P, hh, Z, nz, xe, s, ze, trace)) { memcpy(x, xe, sizeof(double) * n); flag = 0; early_done = 1; st_exit = ORC_EXIT_CONVERGED; __atomic_add_fetch(&orc_early_stats[1], 1, __ATOMIC_RELAXED); break; }
            __atomic_add_fetch(&orc_early_stats[0], 1, __ATOMIC_RELAXED);
        }
        /* near the optimum: primal and complementarity met, dual residual within 100x of its
         * threshold.  An inertia shift or a blocked step from here is the condensed system's
         * round-off (W = z/s ~ 1e14 swamps the soft curvature), not progress: ACCEPTABLE (4) */
        const int near = nrz < th && nry < th && sz / m < fmu * tol && nrx < facc * fx * th * gmax;
        /* a solve that reached the near-optimal region and then left it is past its round-off
         * floor: ACCEPTABLE at the best near-optimal iterate */
        if (saved && !near) { restore = 1; flag = 4; st_exit = ORC_EXIT_LEFT_NEAR; break; }
        /* the saved iterate is the best near-optimal one (smallest scaled dual residual); the
         * polish starts from its s, z too */
        if (near && nrx / gmax <= best_rx) {
            best_rx = nrx / gmax;
            memcpy(xsave, x, sizeof(double) * n); memcpy(ssave, s, sizeof(double) * m); memcpy(zsave, z, sizeof(double) * m);
            saved = 1;
        }
        if (near && ++npassed >= nearwait) { flag = 4; st_exit = ORC_EXIT_NEAR_WAIT; break; }
        for (int r = 0; r < m; r++) { lam[r] = sqrt(s[r] * z[r]); wgt[r] = s[r] / z[r]; }
        double mu = dotv(lam, lam, m) / m;

        /* Hl + J'W^-1 J (full space); hdiag = Lagrangian-Hessian terms beyond Q_qp */
        memset(Hl, 0, sizeof(double) * n * n);
        for (int j = 0; j < n; j++) { Hl[j * n + j] = Pd[j]; hdiag[j] = 0.0; }
        for (int k = 0; k < P.N; k++) {
            double zs = 0;
            for (int j = 0; j < P.K; j++) zs += z[P.mq + k * P.K + j];
            hdiag[4 * k] = -2 * zs; hdiag[4 * k + 2] = -2 * zs;
            Hl[(4 * k) * n + 4 * k] -= 2 * zs; Hl[(4 * k + 2) * n + 4 * k + 2] -= 2 * zs;
        }
        for (int r = 0; r < m; r++) {
            double iw = 1.0 / wgt[r];
            for (int a = 0; a < 4; a++) {
                int ia = Ji[4 * r + a]; if (ia < 0) continue;
                for (int bb = 0; bb < 4; bb++) { int ib = Ji[4 * r + bb]; if (ib < 0) continue; Hl[ia * n + ib] += iw * Jv[4 * r + a] * Jv[4 * r + bb]; }
            }
        }
        /* inertia correction: reduced Hessian Z'(H + delta I)Z must be PD */
        double delta = 0.0, dstart = 0.0; int ok = 0, ntried = 0;
        for (int tries = 0; tries < 14; tries++) {
            for (int i = 0; i < n; i++)
                for (int a = 0; a < nz; a++) {
                    double sacc = 0;
                    for (int j = 0; j < n; j++) sacc += Hl[i * n + j] * Z[(size_t)j * nz + a];
                    HZ[(size_t)i * nz + a] = sacc + delta * Z[(size_t)i * nz + a];
                }
            for (int a = 0; a < nz; a++)
                for (int bb = 0; bb < nz; bb++) {
                    double sacc = 0;
                    for (int i = 0; i < n; i++) sacc += Z[(size_t)i * nz + a] * HZ[(size_t)i * nz + bb];
                    Hr[a * nz + bb] = sacc;
                }
            if (tries == 0) {   /* scale-aware first shift: 1e-10 * max(1, max diag of Z'HZ) */
                dstart = 1.0;
                for (int a = 0; a < nz; a++) if (Hr[a * nz + a] > dstart) dstart = Hr[a * nz + a];
                dstart *= 1e-10;
            }
            if (delta > st_max_delta) st_max_delta = delta;
            if (orc_chol(nz, Hr) == 0) { ok = 1; break; }
            delta = (delta == 0.0) ? dstart : delta * 10.0;
            ntried++;
        }
        if (ntried) { st_shift_iters++; st_failed += ntried; if (ntried > st_max_tries) st_max_tries = ntried; }
        if (!ok) { flag = 1; st_exit = ORC_EXIT_TRIES; break; }
        if (near && delta != 0.0) { flag = 4; st_exit = ORC_EXIT_NEAR_SHIFTED; break; }
        /* full-space KKT [H + delta I, A'; A, 0] */
        memset(K, 0, sizeof(double) * dim * dim);
        for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) K[i * dim + j] = Hl[i * n + j]; K[i * dim + i] += delta; }
        for (int k = 0; k < p; k++) for (int j = 0; j < n; j++) { K[(n + k) * dim + j] = A[(size_t)k * n + j]; K[j * dim + n + k] = A[(size_t)k * n + j]; }
        if (orc_lu(dim, K, piv)) { flag = 1; st_exit = ORC_EXIT_LU; break; }

        for (int pass = 0; pass < 2; pass++) {
            if (pass == 0) for (int r = 0; r < m; r++) ds[r] = -lam[r] * lam[r];
            for (int r = 0; r < m; r++) r3[r] = rz[r] - ds[r] / z[r];
            for (int j = 0; j < n; j++) rhs[j] = rx[j];
            for (int r = 0; r < m; r++) for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) rhs[Ji[4 * r + t]] += Jv[4 * r + t] * r3[r] / wgt[r];
            for (int k = 0; k < p; k++) rhs[n + k] = ry[k];
            orc_lu_solve(dim, K, piv, rhs);
            for (int j = 0; j < n; j++) dx[j] = rhs[j];
            for (int r = 0; r < m; r++) {
                double jd = 0;
                for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) jd += Jv[4 * r + t] * dx[Ji[4 * r + t]];
                dz[r] = (jd - r3[r]) / wgt[r];
                dsv[r] = (ds[r] - s[r] * dz[r]) / z[r];
            }
            if (pass == 0) {
                double ap = steplen(s, dsv, m), ad = steplen(z, dz, m), num = 0;
                for (int r = 0; r < m; r++) num += (s[r] + ap * dsv[r]) * (z[r] + ad * dz[r]);
                double rho = num / dotv(s, z, m), mr = rho < 1 ? rho : 1;
                double sigma = mr * mr * mr; if (sigma < 0) sigma = 0;
                tr_sigma = sigma;
                for (int r = 0; r < m; r++) ds[r] = -(lam[r] * lam[r]) - dsv[r] * dz[r] + sigma * mu;
            } else {
                /* A'dy from the first block row of the Newton system,
                 *   A'dy = rx - (Q_qp + hess + delta I) dx - J'dz,
                 * rather than from the LU's dy: identical in exact arithmetic, but near
                 * convergence the full-space KKT has condition ~1e12 (active rows carry
                 * z/s ~ 1e10) and the LU's dy is only good to ~1e-4 relative, which would
                 * stall ||rx|| above the 1e-6 exit threshold. */
                for (int j = 0; j < n; j++) dq[j] = rx[j] - (Pd[j] + hdiag[j] + delta) * dx[j];
                for (int r = 0; r < m; r++)
                    for (int t = 0; t < 4; t++) if (Ji[4 * r + t] >= 0) dq[Ji[4 * r + t]] -= Jv[4 * r + t] * dz[r];
            }
        }
        double ap = steplen(s, dsv, m), ad = steplen(z, dz, m);
        if (trace)
            fprintf(stderr, "  %2d %10.3e %10.3e %10.3e %10.3e %10.3e %10.3e %10.3e %10.3e\n", iter, nrx, th * gmax, nrz, sz / m,
                    ap, ad, delta, tr_sigma);
        if (near && (ap < ORC_NLP_BLOCKED || ad < ORC_NLP_BLOCKED)) { flag = 4; st_exit = ORC_EXIT_NEAR_BLOCKED; break; }
        ap = 0.99 * ap < 1.0 ? 0.99 * ap : 1.0;
        ad = 0.99 * ad < 1.0 ? 0.99 * ad : 1.0;
        dxlast = 0.0;
        for (int j = 0; j < n; j++) { x[j] += ap * dx[j]; q[j] += ad * dq[j]; dxlast = fmax(dxlast, fabs(ap * dx[j])); }
        for (int r = 0; r < m; r++) { s[r] += ap * dsv[r]; z[r] += ad * dz[r]; }
        it++;
    }
    if (orc_stats_sink) {
        orc_stats_sink[ORC_ST_SHIFT_ITERS] = st_shift_iters; orc_stats_sink[ORC_ST_FAILED] = st_failed;
        orc_stats_sink[ORC_ST_MAX_TRIES] = st_max_tries; orc_stats_sink[ORC_ST_MAX_DELTA] = st_max_delta;
        orc_stats_sink[ORC_ST_EXIT] = st_exit; orc_stats_sink[ORC_ST_POLISH_NPD] = 0.0;
    }
    if (flag == 0 && provisional) flag = 4;
    if (saved && !provisional && (restore || flag == 2 || flag == 4)) {   /* ACCEPTABLE / MAXIT: the best saved iterate */
        memcpy(x, xsave, sizeof(double) * n); memcpy(s, ssave, sizeof(double) * m); memcpy(z, zsave, sizeof(double) * m);
        flag = 4;
    }
#ifdef ORC_DIAG_ENV
    if (getenv("ORC_POLISH_RHO")) g_polish_rho = atof(getenv("ORC_POLISH_RHO"));
    if (getenv("ORC_POLISH_ZINIT")) g_polish_zinit = atoi(getenv("ORC_POLISH_ZINIT"));
    if (getenv("ORC_POLISH_KAPPA")) g_polish_kappa = atof(getenv("ORC_POLISH_KAPPA"));
    if (getenv("ORC_POLISH_IT")) g_polish_it = atoi(getenv("ORC_POLISH_IT"));
    if (getenv("ORC_POLISH_PASSES")) g_polish_passes = atoi(getenv("ORC_POLISH_PASSES"));
    if (getenv("ORC_POLISH_OMCAP")) g_polish_omcap = atof(getenv("ORC_POLISH_OMCAP"));
#endif
    const int do_polish = pp->polish;   /* orc_params.polish (a parameter, not the environment: ADVICE r04) */
    if (do_polish && !early_done && (flag == 0 || flag == 4 || flag == 2) && polish(&P, hh, Z, nz, x, s, z, trace)) flag = 0;
    free(xe); free(ze);
    memcpy(x_out, x, sizeof(double) * n);
    if (iters_out) *iters_out = it;
    free(xsave); free(ssave); free(zsave);
    free(P.gnz); free(P.gval); free(hh); free(x); free(q); free(s); free(z); free(g); free(Jv); free(Ji);
    free(rx); free(ry); free(rz); free(lam); free(wgt); free(ds); free(dsv); free(dz); free(r3); free(K); free(Hl);
    free(rhs); free(dx); free(dq); free(hdiag); free(Z); free(Hr); free(HZ); free(piv);
    return flag;
}
