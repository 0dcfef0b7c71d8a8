// Disturbed plant of the SRB-12 rollout (srb12_plant; DESIGN.md 3 "Disturbed plant", 9, 10.13).  Compiled as part of
// srb12_sim.hip, whose sim12_advance_body derives everything an advance writes from the state it is handed.  Two
// launches per cycle c > c_first (the host launches srb12_sim_advance_kernel at c_first), because the advance is one
// thread per (agent, grid) and a roll inside it would race with the grid-0 thread's stores:
//   srb12_plant_state_kernel         one thread per agent: state[a] <- z + d and the dist_log row.  z is the nominal
//                                    prediction X at grid index 3 or, with `roll`, four forward-Euler steps of the
//                                    plant's own body from the previous cycle's start state (still in `state`) under
//                                    the inputs, footholds and contact flags of that cycle; d is the cycle's kick and
//                                    pushes
//   srb12_sim_advance_plant_kernel   the advance, its state read from `state`
// No LDS, no barrier.  All arithmetic is fp64 with contraction off (srb12_sim.hip's pragma) and every expression is
// written with the grouping of tests/plant12_oracle.py, which restates the kernels in numpy: bit for bit, except what
// passes through cos / sin (the roll).  Groupings (sums are left to right unless bracketed):
//   the world inertia  Ibs = s_g Ib entry by entry; T = Rz Ibs and Iw = T Rz' with every entry (a b + c d) + e f, the
//                      inverse by cofactors over one reciprocal of the determinant: srb12_agent's model prologue and
//                      orc12_dynamics operation for operation
//   a step             p'_i = p_i + Ts v_i
//                      Th'_i = Th_i + (((Ts R[0][i]) w_0 + (Ts R[1][i]) w_1) + (Ts R[2][i]) w_2)
//                      v'_i = v_i + fv_i, then v'_2 <- v'_2 + (-(Ts grav));  fv_i = 0, then per leg in contact, in leg
//                            order, fv_i <- fv_i + (Ts / m_g) f_li
//                      w'_i = w_i + fw_i;  fw_i = 0, then per leg in contact, j = 0 .. 2, fw_i <- fw_i + W_ij f_lj with
//                            W_ij = Ts ((Iwi[i][0] S[0][j] + Iwi[i][1] S[1][j]) + Iwi[i][2] S[2][j]), S = [foot - p^]x
//   the disturbance    d = +0.0; d <- d + bound * u (one rounded multiply, one rounded add); d <- d + push_dv
//   the state          z + d, one rounded add per component
#include "srb_philox.h"

// one forward-Euler step of orc12_dynamics' map about (psi, ph): z <- A z + B u + c, contact 0 legs left out
__device__ __forceinline__ void plant12_step(double z[12], const double psi, const double ph0, const double ph1,
                                             const double ph2, const double Ts, const double tm, const double tg,
                                             const double Ibs[9], const double *__restrict__ u,
                                             const double *__restrict__ fp, const int *__restrict__ ct)
{
    const double c = cos(psi), s = sin(psi);
    const double R[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
    double T[9], Iw[9], Iwi[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[3 * i + j] = R[3 * i] * Ibs[j] + R[3 * i + 1] * Ibs[3 + j] + R[3 * i + 2] * Ibs[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Iw[3 * i + j] = T[3 * i] * R[3 * j] + T[3 * i + 1] * R[3 * j + 1] + T[3 * i + 2] * R[3 * j + 2];
    {
        const double a = Iw[0], b = Iw[1], cc = Iw[2], d = Iw[3], ee = Iw[4], f = Iw[5], g = Iw[6], h = Iw[7], ii = Iw[8];
        const double A0 = ee * ii - f * h, B0 = -(d * ii - f * g), C0 = d * h - ee * g;
        const double r = 1.0 / (a * A0 + b * B0 + cc * C0);
        Iwi[0] = A0 * r; Iwi[1] = -(b * ii - cc * h) * r; Iwi[2] = (b * f - cc * ee) * r;
        Iwi[3] = B0 * r; Iwi[4] = (a * ii - cc * g) * r; Iwi[5] = -(a * f - cc * d) * r;
        Iwi[6] = C0 * r; Iwi[7] = -(a * h - b * g) * r; Iwi[8] = (a * ee - b * d) * r;
    }
    double fv[3] = {0.0, 0.0, 0.0}, fw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 4; l++) {
        if (!ct[l]) continue;
        const double r0 = fp[3 * l] - ph0, r1 = fp[3 * l + 1] - ph1, r2 = fp[3 * l + 2] - ph2;
        const double S[9] = {0.0, -r2, r1, r2, 0.0, -r0, -r1, r0, 0.0};
        const double f[3] = {u[3 * l], u[3 * l + 1], u[3 * l + 2]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            fv[i] = fv[i] + tm * f[i];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double W = Ts * (Iwi[3 * i] * S[j] + Iwi[3 * i + 1] * S[3 + j] + Iwi[3 * i + 2] * S[6 + j]);
                fw[i] = fw[i] + W * f[j];
            }
        }
    }
    double zn[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        zn[i] = z[i] + Ts * z[6 + i];
        zn[3 + i] = z[3 + i] + (((Ts * R[i]) * z[9] + (Ts * R[3 + i]) * z[10]) + (Ts * R[6 + i]) * z[11]);
        zn[6 + i] = z[6 + i] + fv[i];
        zn[9 + i] = z[9 + i] + fw[i];
    }
    zn[8] = zn[8] + tg;
#pragma unroll
    for (int i = 0; i < 12; i++) z[i] = zn[i];
}

extern "C" __global__ void __launch_bounds__(256) srb12_plant_state_kernel(
    int n_agents, int N, double Ts, double mass, Srb12PlantIb Ib, double grav, int c, int c_first,
    double *__restrict__ state, const double *__restrict__ x, const double *__restrict__ xref,
    const double *__restrict__ foot, const int *__restrict__ contact, int agent_offset, unsigned seed_lo,
    unsigned seed_hi, const double *__restrict__ kick_v, const double *__restrict__ kick_p,
    const double *__restrict__ kick_w, const double *__restrict__ plant_mass, const double *__restrict__ plant_inertia,
    int at_state, int roll, int n_push, const int *__restrict__ push_cycle, const int *__restrict__ push_agent,
    const double *__restrict__ push_dv, double *__restrict__ dist_log)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_agents) return;
    const int g = agent_offset + a;                       // the row of the tables, and of the draws
    const int nv = 24 * N + 1;
    const double *xa = x + (size_t)a * nv;
    double *sa = state + 12 * (size_t)a;

    // the base state: the model's prediction, or the plant's own body rolled over the domain from the state that
    // started the previous cycle (still in `state`) under the inputs the model applied
    double z[12];
    if (roll) {
        const double m = plant_mass ? plant_mass[g] : mass, sc = plant_inertia ? plant_inertia[g] : 1.0;
        double Ibs[9];
#pragma unroll
        for (int i = 0; i < 9; i++) Ibs[i] = sc * Ib.v[i];
        const double tm = Ts / m, tg = -(Ts * grav);
#pragma unroll
        for (int i = 0; i < 12; i++) z[i] = sa[i];
        const double *xr = xref + (size_t)a * N * 12;
        const double *fa = foot + (size_t)a * N * 12;
        const int *ca = contact + (size_t)a * N * 4;
        for (int k = 0; k < SIM12_NDOMAIN; k++) {
            // the linearisation point: the plant's own state, or the model's (the start state, then the reference)
            // (no pointer chosen between the registers and global memory: that would be a flat access to scratch)
            double psi = z[5], ph0 = z[0], ph1 = z[1], ph2 = z[2];
            if (!at_state && k > 0) {
                const double *ph = xr + 12 * (k - 1);
                psi = ph[5]; ph0 = ph[0]; ph1 = ph[1]; ph2 = ph[2];
            }
            plant12_step(z, psi, ph0, ph1, ph2, Ts, tm, tg, Ibs, xa + 12 * N + 12 * k, fa + 12 * k, ca + 4 * k);
        }
    } else {
        const double *X3 = xa + 12 * (SIM12_NDOMAIN - 1);
#pragma unroll
        for (int i = 0; i < 12; i++) z[i] = X3[i];
    }

    // the disturbance in state order (only p_x, p_y, v and omega are ever non-zero): the cycle's kicks, then the
    // pushes in table order
    double dpx = 0.0, dpy = 0.0, dv[3] = {0.0, 0.0, 0.0}, dw[3] = {0.0, 0.0, 0.0};
    if (kick_v || kick_p) {
        unsigned w[4];
        plant_philox((unsigned)c, (unsigned)g, 0u, 0u, seed_lo, seed_hi, w);
        if (kick_v) {
            const double b = kick_v[g];
            dv[0] = dv[0] + b * plant_uniform(w[0]);
            dv[1] = dv[1] + b * plant_uniform(w[1]);
        }
        if (kick_p) {
            const double b = kick_p[g];
            dpx = dpx + b * plant_uniform(w[2]);
            dpy = dpy + b * plant_uniform(w[3]);
        }
    }
    if (kick_w) {
        unsigned w[4];
        plant_philox((unsigned)c, (unsigned)g, 1u, 0u, seed_lo, seed_hi, w);
        const double b = kick_w[g];
#pragma unroll
        for (int i = 0; i < 3; i++) dw[i] = dw[i] + b * plant_uniform(w[i]);
    }
    // (both keys loaded before either is tested, four entries a trip: the table is wave-uniform, so these are
    // scalar loads, and a short-circuit would wait for each in turn)
#pragma unroll 4
    for (int p = 0; p < n_push; p++) {
        const int pc = push_cycle[p], pa = push_agent[p];
        if ((pc == c) & (pa == g)) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                dv[i] = dv[i] + push_dv[6 * p + i];
                dw[i] = dw[i] + push_dv[6 * p + 3 + i];
            }
        }
    }

    const double d[12] = {dpx, dpy, 0.0, 0.0, 0.0, 0.0, dv[0], dv[1], dv[2], dw[0], dw[1], dw[2]};
#pragma unroll
    for (int i = 0; i < 12; i++) sa[i] = z[i] + d[i];
    if (dist_log) {
        double *dl = dist_log + ((size_t)(c - c_first - 1) * (size_t)n_agents + a) * 12;
#pragma unroll
        for (int i = 0; i < 12; i++) dl[i] = d[i];
    }
}

extern "C" __global__ void __launch_bounds__(256) srb12_sim_advance_plant_kernel(
    int n_agents, int N, double Ts, double vref, double hcom, double yaw_step, double hold_radius, int gait, int c,
    int c_first, double *__restrict__ state, const double *__restrict__ goal, const int *__restrict__ phase,
    const double *__restrict__ x, const int *__restrict__ status, const int *__restrict__ iters,
    double *__restrict__ x0, double *__restrict__ xref, double *__restrict__ foot, int *__restrict__ contact,
    double *__restrict__ last_state, double *__restrict__ com, double *__restrict__ traj,
    int *__restrict__ status_log, int *__restrict__ iters_log, double *__restrict__ x_log)
{
    sim12_advance_body<true>(n_agents, N, Ts, vref, hcom, yaw_step, hold_radius, gait, c, c_first, state, goal, phase, x,
                             status, iters, x0, xref, foot, contact, last_state, com, traj, status_log, iters_log, x_log);
}
