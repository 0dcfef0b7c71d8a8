// Closed-loop team rollout on the device: the step from one control cycle's solution to the
// next cycle's solver inputs, and the team's safety metrics, so that T cycles run without a host round trip.
//   srb_sim_advance_kernel   one thread per agent: the nominal plant (the next state is the solution's X at grid
//                            index 3, the end of the gait domain -- what the reference buffers, MPC_dist.cpp:798),
//                            the goal-directed reference and trot footholds of workload.make_batch re-centred on
//                            the new position, last cycle's plans shifted by one domain, and the logs; all but the
//                            choice of the state is sim_advance_from_state, which srb_plant.hip (included below:
//                            srb_sim_advance_plant_kernel, the disturbed plant) calls with a state of its own
//   srb_sim_metrics_kernel   brute force over the obstacle table and the neighbour snapshot: nearest obstacle,
//                            nearest other agent, their running minima and the reference's distance_to_fail
//                            (updateDistance_to_fail, MPC_dist.cpp:21-40); its scan and its update rules are in
//                            srb_sim_scan.h, shared with the per-scene kernel of srb_scenes.hip
// One cycle is one gait domain of NDOMAIN = 4 grids (global_loco_opts.h:9).  All arithmetic is fp64 with
// contraction off and every expression is written with the grouping of tests/sim_oracle.py, which restates both
// kernels in numpy bit for bit.
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_decls.h"

#pragma clang fp contract(off)

#define SIM_NDOMAIN 4

// MPC_dist.cpp:1206-1209: FR, FL, RR, RL offsets of the default stance (as srb_prepare.hip)
__constant__ double c_sim_foot[4][2] = {{0.2188, -0.1320}, {0.2188, 0.1320}, {-0.1472, -0.1320}, {-0.1472, 0.1320}};

// What an advance derives from the state (px, vx, py, vy) that starts cycle c, for agent a of A: alpha_buf, x0, the
// snapshot row, the reference, the footholds, the traj row, and for c != c_first last cycle's plans shifted and the
// previous solve's logs.  xa: the agent's previous decision vector (null at c_first).  Shared by the nominal
// advance below and the disturbed plant of srb_plant.hip, which differ in the state they hand in.
__device__ __forceinline__ void sim_advance_from_state(
    const int a, const size_t A, const int N, const int C, const int nv, const double Ts, const double vref,
    const int c, const int c_first, const double px, const double vx, const double py, const double vy,
    const double *goal, const int *phase, const double *xa,
    const int *status, const int *iters, double *x0, double *ref,
    double *foot, double *last_state, double *alpha_buf,
    double *plan_table, double *traj, int *status_log,
    int *iters_log, double *x_log)
{
    if (alpha_buf) {
        double *ab = alpha_buf + 4 * (size_t)a;
        ab[0] = px; ab[1] = vx; ab[2] = py; ab[3] = vy;
    }
    double *o = x0 + 4 * (size_t)a;
    o[0] = px; o[1] = vx; o[2] = py; o[3] = vy;
    o = last_state + 4 * (size_t)a;                       // the snapshot row layout (get_lastState)
    o[0] = px; o[1] = py; o[2] = vx; o[3] = vy;

    // the reference: a straight line to the goal at min(vref, the speed that arrives at the horizon's end)
    const double dx = goal[2 * (size_t)a] - px, dy = goal[2 * (size_t)a + 1] - py;
    const double dist = sqrt(dx * dx + dy * dy);
    const double ux = dist > 0.0 ? dx / dist : 0.0, uy = dist > 0.0 ? dy / dist : 0.0;
    const double q = dist / (Ts * (double)N);
    const double v = q < vref ? q : vref;
    const double wx = ux * v, wy = uy * v;
    double *ra = ref + (size_t)a * 4 * N;
    for (int k = 0; k < N; k++) {
        const double t = Ts * (double)(k + 1);
        ra[4 * k + 0] = px + wx * t;
        ra[4 * k + 1] = wx;
        ra[4 * k + 2] = py + wy * t;
        ra[4 * k + 3] = wy;
    }

    // the footholds: the default stance around the reference position at each domain's start, one trot
    // diagonal per domain ({FR,RL} on even parity), all four legs for C = 4
    const int par0 = c + (phase ? phase[a] : 0);
    double *fa = foot + (size_t)a * N * 2 * C;
    for (int k = 0; k < N; k++) {
        const int j = k / SIM_NDOMAIN;
        const double t = Ts * (double)(SIM_NDOMAIN * j);
        const double cx = px + wx * t, cy = py + wy * t;
        const bool odd = ((par0 + j) & 1) != 0;
        for (int i = 0; i < C; i++) {
            const int leg = C == 2 ? (odd ? 1 + i : 3 * i) : i;        // {FL,RR} = 1, 2; {FR,RL} = 0, 3
            fa[(size_t)k * 2 * C + i] = c_sim_foot[leg][0] + cx;
            fa[(size_t)k * 2 * C + C + i] = c_sim_foot[leg][1] + cy;
        }
    }

    const int r = c - c_first;                            // row of the logs
    if (traj) {
        double *t = traj + ((size_t)r * A + a) * 4;
        t[0] = px; t[1] = vx; t[2] = py; t[3] = vy;
    }
    if (c == c_first) return;

    // last cycle's plans as this cycle's table (dist.shift_plans(., 4)): grid k is the old grid k + 4, and
    // past the horizon the last finite difference goes on, last + m (last - previous)
    if (plan_table) {
        double *pt = plan_table + (size_t)a * 2 * N;
        const double lx = xa[4 * (N - 1)], ly = xa[4 * (N - 1) + 2];
        const double ex = lx - xa[4 * (N - 2)], ey = ly - xa[4 * (N - 2) + 2];
        for (int k = 0; k < N; k++) {
            if (k + SIM_NDOMAIN < N) {
                pt[2 * k] = xa[4 * (k + SIM_NDOMAIN)];
                pt[2 * k + 1] = xa[4 * (k + SIM_NDOMAIN) + 2];
            } else {
                const double m = (double)(k + SIM_NDOMAIN - N + 1);
                pt[2 * k] = lx + m * ex;
                pt[2 * k + 1] = ly + m * ey;
            }
        }
    }
    // the previous solve's outputs
    if (status_log && status) {
        status_log[((size_t)(r - 1) * A + a) * 2] = status[2 * (size_t)a];
        status_log[((size_t)(r - 1) * A + a) * 2 + 1] = status[2 * (size_t)a + 1];
    }
    if (iters_log && iters) {
        iters_log[((size_t)(r - 1) * A + a) * 2] = iters[2 * (size_t)a];
        iters_log[((size_t)(r - 1) * A + a) * 2 + 1] = iters[2 * (size_t)a + 1];
    }
    if (x_log) {
        double *xl = x_log + ((size_t)(r - 1) * A + a) * nv;
        for (int i = 0; i < nv; i++) xl[i] = xa[i];
    }
}

extern "C" __global__ void __launch_bounds__(256) srb_sim_advance_kernel(
    int n_agents, int N, int C, int nv, double Ts, double vref, int c, int c_first, double *__restrict__ state,
    const double *__restrict__ goal, const int *__restrict__ phase, const double *__restrict__ x,
    const int *__restrict__ status, const int *__restrict__ iters, double *__restrict__ x0, double *__restrict__ ref,
    double *__restrict__ foot, double *__restrict__ last_state, double *__restrict__ alpha_buf,
    double *__restrict__ plan_table, double *__restrict__ traj, int *__restrict__ status_log,
    int *__restrict__ iters_log, double *__restrict__ x_log)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_agents) return;
    const size_t A = (size_t)n_agents;
    const double *xa = x ? x + (size_t)a * nv : nullptr;
    double *sa = state + 4 * (size_t)a;
    // the state: the caller's before the first solve, else X at grid index 3 of the previous solution,
    // whatever its status (a non-optimal exit returns the last iterate, as the reference does)
    double px, vx, py, vy;
    if (c == c_first) {
        px = sa[0]; vx = sa[1]; py = sa[2]; vy = sa[3];
    } else {
        const double *X3 = xa + 4 * (SIM_NDOMAIN - 1);
        px = X3[0]; vx = X3[1]; py = X3[2]; vy = X3[3];
        sa[0] = px; sa[1] = vx; sa[2] = py; sa[3] = vy;
    }
    sim_advance_from_state(a, A, N, C, nv, Ts, vref, c, c_first, px, vx, py, vy, goal, phase, xa, status, iters,
                           x0, ref, foot, last_state, alpha_buf, plan_table, traj, status_log, iters_log, x_log);
}

#include "srb_plant.hip"       // the disturbed plant (srb_plant): srb_sim_advance_plant_kernel, on the body above

#include "srb_sim_scan.h"      // SIM_TILE, SIM_AG, SIM_SL and sim_nearest2, the tiled scan (shared with srb_scenes.hip)

// SIM_AG agents per block of SIM_TILE threads, SIM_SL threads per agent.  (One thread per agent leaves a
// 1024-agent team on 4 CUs, each thread walking every row: 0.156 ms at 5120 obstacles + 1024 agents, half a
// solve.)  A minimum is exact in any order, so the split changes no bit of the result.
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_metrics_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles, int n_obs,
    const double *__restrict__ nbr_state, int n_all, int agent_offset, double *__restrict__ d_obs,
    double *__restrict__ d_agent, double *__restrict__ min_d_obs, double *__restrict__ min_d_agent,
    int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail)
{
    __shared__ double2 tile[SIM_TILE];
    __shared__ double part[2][SIM_SL][SIM_AG];
    const int al = (int)threadIdx.x % SIM_AG, slice = (int)threadIdx.x / SIM_AG;
    const int a = blockIdx.x * SIM_AG + al;
    const bool live = a < n_agents;
    const double px = live ? state[4 * (size_t)a] : 0.0, py = live ? state[4 * (size_t)a + 2] : 0.0;
    double b_ob = sim_nearest2(obstacles, n_obs, 2, -1, px, py, tile);
    double b_ag = sim_nearest2(nbr_state, n_all, 4, agent_offset + a, px, py, tile);
    part[0][slice][al] = b_ob;
    part[1][slice][al] = b_ag;
    __syncthreads();
    if (!live || slice != 0) return;
    for (int s = 1; s < SIM_SL; s++) {
        if (part[0][s][al] < b_ob) b_ob = part[0][s][al];
        if (part[1][s][al] < b_ag) b_ag = part[1][s][al];
    }
    sim_metrics_store(a, c, c_first, px, py, b_ob, b_ag, d_obs, d_agent, min_d_obs, min_d_agent, fail_cycle,
                      distance_to_fail);
}
