// Disturbed plant of the LIP rollout (srb_plant; DESIGN.md 3 "Disturbed plant", 9, 10.12).  Compiled as part of
// srb_sim.hip, whose sim_advance_from_state derives everything an advance writes from the state it is handed.
//   srb_sim_advance_plant_kernel   one thread per agent, cycles c > c_first only (the host launches
//                                  srb_sim_advance_kernel at c_first): the state that starts cycle c is z + d,
//                                  z the nominal prediction X at grid index 3 or, with plant_hcom, the four-step
//                                  roll of the plant's own LIP from the previous cycle's start state, and d the
//                                  cycle's kick and pushes
// All arithmetic is fp64 with contraction off (srb_sim.hip's pragma) and every expression is written with the
// grouping of tests/plant_oracle.py, which restates the kernel in numpy bit for bit.  Groupings:
//   plant_lip          srb_capi.cpp make_kparams operation for operation: every 4x4 product entry is
//                      s = 0; s += X[i][k] * Y[k][j] for k = 0 .. 3;  Ad = ((I + A T) + ((0.5 A2) T) T) + (((A3 T) T) T) / 6;
//                      Bd = (Ai (Ad - I)) B with the same row sums
//   the roll           z_i <- ((((Ad[i][0] z0 + Ad[i][1] z1) + Ad[i][2] z2) + Ad[i][3] z3) + Bd[i][0] u0) + Bd[i][1] u1:
//                      a row sum in index order, Ad's terms then Bd's, from the first product (no leading zero);
//                      (u0, u1) of step k is U_k = x[4N + 2k], x[4N + 2k + 1], the input of the equality row
//                      X_k = Ad X_{k-1} + Bd U_k (oracle/problem.c), k = 0 .. 3
//   the disturbance    d = +0.0; d <- d + bound * u (one rounded multiply, one rounded add); d <- d + push_dv
//   the state          z + d, one rounded add per component

// Philox4x32-10 and the word -> (-1, 1) conversion: srb_philox.h, shared with srb12_plant.hip
#include "srb_philox.h"

__device__ __forceinline__ void plant_mm4(const double *X, const double *Y, double *Z)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) s += X[i * 4 + k] * Y[k * 4 + j];
            Z[i * 4 + j] = s;
        }
}

// Ad [4][4], Bd [4][2] of the LIP with w2 = grav / hcom and step T (make_kparams, srb_capi.cpp)
__device__ __forceinline__ void plant_lip(const double w2, const double T, double *Ad, double *Bd)
{
    double A[16] = {0}, B[8] = {0}, A2[16], A3[16];
    A[1] = 1; A[4] = w2; A[11] = 1; A[14] = w2;
    B[2] = -w2; B[7] = -w2;
    plant_mm4(A, A, A2); plant_mm4(A2, A, A3);
#pragma unroll
    for (int i = 0; i < 16; i++) Ad[i] = (i % 5 == 0 ? 1.0 : 0.0) + A[i] * T + 0.5 * A2[i] * T * T + A3[i] * T * T * T / 6;
    double Ai[16] = {0}, AdI[16], M[16];
    Ai[1] = 1.0 / w2; Ai[4] = 1.0; Ai[11] = 1.0 / w2; Ai[14] = 1.0;
#pragma unroll
    for (int i = 0; i < 16; i++) AdI[i] = Ad[i] - (i % 5 == 0 ? 1.0 : 0.0);
    plant_mm4(Ai, AdI, M);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            double s = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) s += M[i * 4 + q] * B[q * 2 + j];
            Bd[i * 2 + j] = s;
        }
}

extern "C" __global__ void __launch_bounds__(256) srb_sim_advance_plant_kernel(
    int n_agents, int N, int C, int nv, double Ts, double vref, int c, int c_first, double *__restrict__ state,
    const double *__restrict__ goal, const int *__restrict__ phase, const double *__restrict__ x,
    const int *__restrict__ status, const int *__restrict__ iters, double *__restrict__ x0, double *__restrict__ ref,
    double *__restrict__ foot, double *__restrict__ last_state, double *__restrict__ alpha_buf,
    double *__restrict__ plan_table, double *__restrict__ traj, int *__restrict__ status_log,
    int *__restrict__ iters_log, double *__restrict__ x_log, int agent_offset, double grav, unsigned seed_lo,
    unsigned seed_hi, const double *__restrict__ kick_v, const double *__restrict__ kick_p,
    const double *__restrict__ plant_hcom, int n_push, const int *__restrict__ push_cycle,
    const int *__restrict__ push_agent, const double *__restrict__ push_dv, double *__restrict__ dist_log)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_agents) return;
    const int g = agent_offset + a;                       // the row of the tables, and of the draws
    const double *xa = x + (size_t)a * nv;
    double *sa = state + 4 * (size_t)a;

    // the base state: the model's prediction, or the plant's own LIP rolled over the domain from the state
    // that started the previous cycle (still in `state`) under the inputs the model applied
    double z0, z1, z2, z3;
    if (plant_hcom) {
        double Ad[16], Bd[8];
        plant_lip(grav / plant_hcom[g], Ts, Ad, Bd);
        z0 = sa[0]; z1 = sa[1]; z2 = sa[2]; z3 = sa[3];
        for (int k = 0; k < SIM_NDOMAIN; k++) {
            const double u0 = xa[4 * N + 2 * k], u1 = xa[4 * N + 2 * k + 1];
            double zn[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
                zn[i] = ((((Ad[4 * i] * z0 + Ad[4 * i + 1] * z1) + Ad[4 * i + 2] * z2) + Ad[4 * i + 3] * z3) +
                         Bd[2 * i] * u0) + Bd[2 * i + 1] * u1;
            z0 = zn[0]; z1 = zn[1]; z2 = zn[2]; z3 = zn[3];
        }
    } else {
        const double *X3 = xa + 4 * (SIM_NDOMAIN - 1);
        z0 = X3[0]; z1 = X3[1]; z2 = X3[2]; z3 = X3[3];
    }

    // the disturbance (dpx, dvx, dpy, dvy): the cycle's kick, then the pushes in table order
    double dpx = 0.0, dvx = 0.0, dpy = 0.0, dvy = 0.0;
    if (kick_v || kick_p) {
        unsigned w[4];
        plant_philox((unsigned)c, (unsigned)g, 0u, 0u, seed_lo, seed_hi, w);
        if (kick_v) {
            const double b = kick_v[g];
            dvx = dvx + b * plant_uniform(w[0]);
            dvy = dvy + b * plant_uniform(w[1]);
        }
        if (kick_p) {
            const double b = kick_p[g];
            dpx = dpx + b * plant_uniform(w[2]);
            dpy = dpy + b * plant_uniform(w[3]);
        }
    }
    // (both keys loaded before either is tested, four entries a trip: the table is wave-uniform, so these are
    // scalar loads, and a short-circuit would wait for each in turn)
#pragma unroll 4
    for (int p = 0; p < n_push; p++) {
        const int pc = push_cycle[p], pa = push_agent[p];
        if ((pc == c) & (pa == g)) {
            dvx = dvx + push_dv[2 * p];
            dvy = dvy + push_dv[2 * p + 1];
        }
    }

    const double px = z0 + dpx, vx = z1 + dvx, py = z2 + dpy, vy = z3 + dvy;
    sa[0] = px; sa[1] = vx; sa[2] = py; sa[3] = vy;
    if (dist_log) {
        double *dl = dist_log + ((size_t)(c - c_first - 1) * (size_t)n_agents + a) * 4;
        dl[0] = dpx; dl[1] = dvx; dl[2] = dpy; dl[3] = dvy;
    }
    sim_advance_from_state(a, (size_t)n_agents, N, C, nv, Ts, vref, c, c_first, px, vx, py, vy, goal, phase, xa, status, iters,
                           x0, ref, foot, last_state, alpha_buf, plan_table, traj, status_log, iters_log, x_log);
}
