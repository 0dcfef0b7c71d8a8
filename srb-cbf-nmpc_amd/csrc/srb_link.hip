// Degraded neighbour link of the LIP rollout (srb_link; DESIGN.md 3 "Degraded link", 9, 10.14): one broadcast per
// agent per cycle, late by delay[g] cycles, lost with probability drop[g], its state noisy by noise_p / noise_v.
//   srb_link_update_kernel<LPR>   one cycle's update of all n_all rows, LPR threads per row: the message of cycle c
//                                 goes into its ring slot, the message of c - delay[g] arrives (or not), and the
//                                 perceived row seen_state[g] / seen_plan[g] is what the receivers hold, dead-reckoned
//                                 by its age with extrapolate.  Launched between the metrics and the solve.
// Rows are independent.  The row's threads all take the same branch (arrival is a function of the row), and what a
// branch reads it does not write: held_cycle and held_plan are read only when nothing arrives and written only when
// something does, the ring slot read (cycle c - delay, delay >= 1) is never the slot written (cycle c), and a message
// of delay 0 is taken from the registers / the plan table, not read back.  So no two threads race on a row, whatever
// LPR.  Thread 0 of a row writes the row's state, cycle and age; the plan grids are strided over the row's threads.
// All arithmetic is fp64 with contraction off and every expression is written with the grouping of
// tests/link_oracle.py, which restates the kernel in numpy bit for bit.  Groupings:
//   noise        m_i = s_i + bound * u_i: one rounded multiply, one rounded add; a null table leaves s_i as it is
//   loss         0.5 * u0 + 0.5 < drop[g] (the left side is exact)
//   dead reckon  p + v * ((double)(4 age) * Ts); age 0 (or extrapolate 0) is a copy
//   plan shift   grid k + 4 age inside the horizon: that grid; beyond: last + (double)(k + 4 age - N + 1) * (last - previous)
//   no plan yet  p + v * (Ts * (double)(k + 1)) from the seen state
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_decls.h"
#include "srb_philox.h"

#pragma clang fp contract(off)

template <int LPR>
__global__ void __launch_bounds__(256) srb_link_update_kernel(
    int n_all, int N, double Ts, int c, int c_first, int max_delay, int slot_c, int extrapolate, unsigned seed_lo,
    unsigned seed_hi, const int *__restrict__ delay, const double *__restrict__ drop, const double *__restrict__ noise_p,
    const double *__restrict__ noise_v, const double *__restrict__ last_state, const double *__restrict__ plan_table,
    double *ring_state, double *ring_plan, double *held_state, double *held_plan, int *held_cycle, double *seen_state,
    double *seen_plan, int *age_row)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / LPR, lane = t % LPR;
    if (g >= n_all) return;
    const size_t row = (size_t)g, np = 2 * (size_t)N;       // np: doubles of a plan row
    const bool plans = plan_table && c > c_first;            // no plan is sent at c_first

    // the message of cycle c: the snapshot row with the sender's noise, into the ring with the row's shifted plan
    double m0 = last_state[4 * row], m1 = last_state[4 * row + 1], m2 = last_state[4 * row + 2],
           m3 = last_state[4 * row + 3];
    if (noise_p || noise_v) {
        unsigned w[4];
        plant_philox((unsigned)c, (unsigned)g, 3u, 0u, seed_lo, seed_hi, w);
        if (noise_p) {
            const double b = noise_p[g];
            m0 = m0 + b * plant_uniform(w[0]);
            m1 = m1 + b * plant_uniform(w[1]);
        }
        if (noise_v) {
            const double b = noise_v[g];
            m2 = m2 + b * plant_uniform(w[2]);
            m3 = m3 + b * plant_uniform(w[3]);
        }
    }
    const double *pt = plans ? plan_table + row * np : nullptr;
    if (lane == 0) {
        double *rs = ring_state + ((size_t)slot_c * n_all + row) * 4;
        rs[0] = m0; rs[1] = m1; rs[2] = m2; rs[3] = m3;
    }
    if (plans) {
        double *rp = ring_plan + ((size_t)slot_c * n_all + row) * np;
        for (int k = lane; k < N; k += LPR) { rp[2 * k] = pt[2 * k]; rp[2 * k + 1] = pt[2 * k + 1]; }
    }

    // what arrives: at c_first the first message, at once; later the message of s = c - delay[g], unless lost
    int d = 0, s = c;
    bool arrive = true;
    if (c > c_first) {
        if (delay) d = min(max(delay[g], 0), max_delay);     // (an entry outside the ring would index outside it)
        s = c - d;
        arrive = s > c_first;
        if (arrive && drop) {
            unsigned w[4];
            plant_philox((unsigned)s, (unsigned)g, 2u, 0u, seed_lo, seed_hi, w);
            arrive = !(0.5 * plant_uniform(w[0]) + 0.5 < drop[g]);
        }
    }

    // the held message after this cycle: the arrival (from the registers and the plan table at delay 0, else from its
    // ring slot) or what was held
    double h0 = m0, h1 = m1, h2 = m2, h3 = m3;
    const double *hp = pt;
    int hc = s;
    if (arrive && d > 0) {
        int slot_s = slot_c - d;
        if (slot_s < 0) slot_s += max_delay + 1;
        const double *rs = ring_state + ((size_t)slot_s * n_all + row) * 4;
        h0 = rs[0]; h1 = rs[1]; h2 = rs[2]; h3 = rs[3];
        hp = ring_plan + ((size_t)slot_s * n_all + row) * np;
    } else if (!arrive) {
        const double *hs = held_state + 4 * row;
        h0 = hs[0]; h1 = hs[1]; h2 = hs[2]; h3 = hs[3];
        hp = held_plan + row * np;
        hc = held_cycle[g];
    }
    const int age = c - hc;
    if (arrive) {
        if (lane == 0) {
            double *hs = held_state + 4 * row;
            hs[0] = h0; hs[1] = h1; hs[2] = h2; hs[3] = h3;
            held_cycle[g] = hc;
        }
        if (plans) {
            double *hw = held_plan + row * np;
            for (int k = lane; k < N; k += LPR) { hw[2 * k] = hp[2 * k]; hw[2 * k + 1] = hp[2 * k + 1]; }
        }
    }

    // what is seen
    const int m = extrapolate ? 4 * age : 0;                 // grids to dead-reckon over
    double e0 = h0, e1 = h1;
    if (m > 0) {
        const double dt = (double)m * Ts;
        e0 = h0 + h2 * dt;
        e1 = h1 + h3 * dt;
    }
    if (lane == 0) {
        double *ss = seen_state + 4 * row;
        ss[0] = e0; ss[1] = e1; ss[2] = h2; ss[3] = h3;
        if (age_row) age_row[g] = age;
    }
    if (!plans) return;
    double *sp = seen_plan + row * np;
    if (hc == c_first) {                                     // no plan held yet: constant velocity from the seen state
        for (int k = lane; k < N; k += LPR) {
            const double tk = Ts * (double)(k + 1);
            sp[2 * k] = e0 + h2 * tk;
            sp[2 * k + 1] = e1 + h3 * tk;
        }
        return;
    }
    const double lx = hp[2 * (N - 1)], ly = hp[2 * (N - 1) + 1];
    const double ex = lx - hp[2 * (N - 2)], ey = ly - hp[2 * (N - 2) + 1];
    for (int k = lane; k < N; k += LPR) {
        const int i = k + m;
        if (i < N) {
            sp[2 * k] = hp[2 * i];
            sp[2 * k + 1] = hp[2 * i + 1];
        } else {
            const double j = (double)(i - N + 1);
            sp[2 * k] = lx + j * ex;
            sp[2 * k + 1] = ly + j * ey;
        }
    }
}

int srb_launch_link_update(int lanes, int n_all, int N, double Ts, int c, int c_first, int max_delay, int slot_c,
                           int extrapolate, unsigned seed_lo, unsigned seed_hi, const int *delay, const double *drop,
                           const double *noise_p, const double *noise_v, const double *last_state,
                           const double *plan_table, double *ring_state, double *ring_plan, double *held_state,
                           double *held_plan, int *held_cycle, double *seen_state, double *seen_plan, int *age_row,
                           hipStream_t s)
{
    const dim3 grid((unsigned)(((size_t)n_all * lanes + 255) / 256)), block(256);
#define SRB_LINK_LAUNCH(L)                                                                                           \
    hipLaunchKernelGGL(srb_link_update_kernel<L>, grid, block, 0, s, n_all, N, Ts, c, c_first, max_delay, slot_c,      \
                       extrapolate, seed_lo, seed_hi, delay, drop, noise_p, noise_v, last_state, plan_table,           \
                       ring_state, ring_plan, held_state, held_plan, held_cycle, seen_state, seen_plan, age_row)
    switch (lanes) {
    case 1: SRB_LINK_LAUNCH(1); break;
    case 8: SRB_LINK_LAUNCH(8); break;
    case 16: SRB_LINK_LAUNCH(16); break;
    default: return 1;
    }
#undef SRB_LINK_LAUNCH
    return 0;
}
