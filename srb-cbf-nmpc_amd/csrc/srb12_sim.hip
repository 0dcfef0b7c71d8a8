// Closed-loop rollout of the SRB-12 mode: the step from one cycle's 12-state solution to the
// next cycle's solver inputs.  srb12_sim_advance_kernel follows srb_sim_advance_kernel (srb_sim.hip) rule for rule:
// the nominal plant (the next state is X at grid index 3 of the previous solution, whatever its status), the
// goal-directed reference line of the LIP rollout, and workload.make_batch12's lift of it -- the height hcom, a
// yaw reference that turns towards the goal by at most yaw_step a cycle, the default stance rotated by that yaw
// around the reference position at each domain's start, and the trot / stand contact flags.  The safety metrics are
// srb_sim_metrics_kernel / srb_sim_scene_metrics_kernel on the `com` rows written here (no copy of the scan).
// One cycle is one gait domain of NDOMAIN = 4 grids.  All arithmetic is fp64 with contraction off and every
// expression is written with the grouping of tests/sim12_oracle.py, which restates the kernel in numpy: bit for
// bit except what passes through atan2, cos and sin (yaw_ref, xref column 5, foot x and y), which are not
// correctly rounded on either side.
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_decls.h"

#pragma clang fp contract(off)

#define SIM12_NDOMAIN 4

// MPC_dist.cpp:1206-1209: FR, FL, RR, RL offsets of the default stance (as srb_sim.hip)
static __constant__ double c_sim12_foot[4][2] = {{0.2188, -0.1320}, {0.2188, 0.1320}, {-0.1472, -0.1320}, {-0.1472, 0.1320}};

// One thread per (agent, grid): thread a N + k writes grid k's rows of xref, foot and contact and every N-th word
// of the x_log row, the thread of grid 0 the per-agent rows.  Each thread derives the agent's reference from the
// state itself (a square root, a division, one atan2 and one sincos: nothing next to its stores), so there is no
// exchange between threads and no barrier.  (One thread per agent writes 24 N + 1 + 28 N words at a stride of
// that many between neighbouring lanes.)
// The body is shared with srb12_sim_advance_plant_kernel (srb12_plant.hip) through FROM_STATE: false, the nominal
// plant (the state of a cycle c > c_first is X at grid index 3 of the previous solution); true, the state is what
// srb12_plant_state_kernel left in `state` (read by every thread of the agent, written by none).
template <bool FROM_STATE>
__device__ __forceinline__ void sim12_advance_body(
    int n_agents, int N, double Ts, double vref, double hcom, double yaw_step, double hold_radius, int gait, int c,
    int c_first, double *__restrict__ state, const double *__restrict__ goal, const int *__restrict__ phase,
    const double *__restrict__ x, const int *__restrict__ status, const int *__restrict__ iters,
    double *__restrict__ x0, double *__restrict__ xref, double *__restrict__ foot, int *__restrict__ contact,
    double *__restrict__ last_state, double *__restrict__ com, double *__restrict__ traj,
    int *__restrict__ status_log, int *__restrict__ iters_log, double *__restrict__ x_log)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = idx / N, k = idx - a * N;
    if (a >= n_agents) return;
    const size_t A = (size_t)n_agents;
    const int nv = 24 * N + 1;
    const double *xa = x ? x + (size_t)a * nv : nullptr;
    // the state: the caller's before the first solve (read only then), else X at grid index 3 of the previous
    // solution, whatever its status
    const double *src = (FROM_STATE || c == c_first) ? state + 12 * (size_t)a : xa + 12 * (SIM12_NDOMAIN - 1);
    double st[12];
    for (int i = 0; i < 12; i++) st[i] = src[i];
    const double px = st[0], py = st[1], yaw = st[5];

    // the reference line of the LIP rollout: straight to the goal at min(vref, the speed that arrives at the
    // horizon's end)
    const double dx = goal[2 * (size_t)a] - px, dy = goal[2 * (size_t)a + 1] - py;
    const double dist = sqrt(dx * dx + dy * dy);
    const double ux = dist > 0.0 ? dx / dist : 0.0, uy = dist > 0.0 ? dy / dist : 0.0;
    const double q = dist / (Ts * (double)N);
    const double v = q < vref ? q : vref;
    const double wx = ux * v, wy = uy * v;

    // the yaw reference, a function of the state alone: towards the goal's bearing the short way round, at most
    // yaw_step a cycle; inside hold_radius the bearing means nothing and the agent keeps its yaw
    const double two_pi = 2.0 * 3.141592653589793;
    double e = atan2(dy, dx) - yaw;
    e = e - two_pi * rint(e / two_pi);
    e = e > yaw_step ? yaw_step : (e < -yaw_step ? -yaw_step : e);
    const double yaw_ref = dist > hold_radius ? yaw + e : yaw;

    double *xr = xref + ((size_t)a * N + k) * 12;
    const double t = Ts * (double)(k + 1);
    xr[0] = px + wx * t;
    xr[1] = py + wy * t;
    xr[2] = hcom;
    xr[3] = 0.0; xr[4] = 0.0;
    xr[5] = yaw_ref;
    xr[6] = wx;
    xr[7] = wy;
    xr[8] = 0.0; xr[9] = 0.0; xr[10] = 0.0; xr[11] = 0.0;

    // the footholds: the stance rotated by yaw_ref around the reference position at the domain's start; contact:
    // all four legs (stand), or one trot diagonal per domain, {FR,RL} on even parity
    const int j = k / SIM12_NDOMAIN;
    const double tj = Ts * (double)(SIM12_NDOMAIN * j);
    const double cx = px + wx * tj, cy = py + wy * tj;
    const double cs = cos(yaw_ref), sn = sin(yaw_ref);
    const bool odd = ((c + (phase ? phase[a] : 0) + j) & 1) != 0;
    double *fa = foot + ((size_t)a * N + k) * 12;
    int *ca = contact + ((size_t)a * N + k) * 4;
    for (int l = 0; l < 4; l++) {
        const double sx = c_sim12_foot[l][0], sy = c_sim12_foot[l][1];
        fa[3 * l + 0] = cx + (cs * sx - sn * sy);
        fa[3 * l + 1] = cy + (sn * sx + cs * sy);
        fa[3 * l + 2] = 0.0;
        ca[l] = gait == 1 ? 1 : ((l == 0 || l == 3) != odd ? 1 : 0);
    }

    const int r = c - c_first;                            // row of the logs
    if (k == 0) {
        if (!FROM_STATE && c != c_first) {
            double *sa = state + 12 * (size_t)a;
            for (int i = 0; i < 12; i++) sa[i] = st[i];
        }
        double *o = x0 + 12 * (size_t)a;
        for (int i = 0; i < 12; i++) o[i] = st[i];
        o = last_state + 4 * (size_t)a;                   // the snapshot row layout (get_lastState)
        o[0] = px; o[1] = py; o[2] = st[6]; o[3] = st[7];
        o = com + 4 * (size_t)a;                          // the row the selection and the metrics scan read
        o[0] = px; o[1] = st[6]; o[2] = py; o[3] = st[7];
        if (traj) {
            o = traj + ((size_t)r * A + a) * 12;
            for (int i = 0; i < 12; i++) o[i] = st[i];
        }
    }
    if (c == c_first) return;

    // the previous solve's outputs
    if (k == 0) {
        if (status_log && status) {
            status_log[((size_t)(r - 1) * A + a) * 2] = status[2 * (size_t)a];
            status_log[((size_t)(r - 1) * A + a) * 2 + 1] = status[2 * (size_t)a + 1];
        }
        if (iters_log && iters) {
            iters_log[((size_t)(r - 1) * A + a) * 2] = iters[2 * (size_t)a];
            iters_log[((size_t)(r - 1) * A + a) * 2 + 1] = iters[2 * (size_t)a + 1];
        }
    }
    if (x_log) {
        double *xl = x_log + ((size_t)(r - 1) * A + a) * nv;
        for (int i = k; i < nv; i += N) xl[i] = xa[i];
    }
}

extern "C" __global__ void __launch_bounds__(256) srb12_sim_advance_kernel(
    int n_agents, int N, double Ts, double vref, double hcom, double yaw_step, double hold_radius, int gait, int c,
    int c_first, double *__restrict__ state, const double *__restrict__ goal, const int *__restrict__ phase,
    const double *__restrict__ x, const int *__restrict__ status, const int *__restrict__ iters,
    double *__restrict__ x0, double *__restrict__ xref, double *__restrict__ foot, int *__restrict__ contact,
    double *__restrict__ last_state, double *__restrict__ com, double *__restrict__ traj,
    int *__restrict__ status_log, int *__restrict__ iters_log, double *__restrict__ x_log)
{
    sim12_advance_body<false>(n_agents, N, Ts, vref, hcom, yaw_step, hold_radius, gait, c, c_first, state, goal, phase, x,
                              status, iters, x0, xref, foot, contact, last_state, com, traj, status_log, iters_log, x_log);
}

// Last cycle's plans as this cycle's table (dist.shift_plans on the device): the new cycle starts `grids` grids
// later, so its grid k is the old grid k + grids; past the horizon the plan goes on along its last finite
// difference, last + m (last - previous) with m = k + grids - N + 1 -- the operation order of
// srb_sim_advance_kernel's shift (srb_sim.hip), contraction off.  One thread per (agent, grid) as the advance
// above; a kernel of its own, so the advance and the plans-off rollout keep their code.  N >= 2, grids >= 0,
// plan and table [n_agents][N][2] distinct buffers (checked by the host).
extern "C" __global__ void __launch_bounds__(256) srb12_plan_shift_kernel(int n_agents, int N, int grids,
                                                                          const double *__restrict__ plan,
                                                                          double *__restrict__ table)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = idx / N, k = idx - a * N;
    if (a >= n_agents) return;
    const double *pa = plan + (size_t)a * 2 * N;
    double *pt = table + ((size_t)a * N + k) * 2;
    // (k + grids < N without the sum: grids is any non-negative int)
    if (grids < N - k) {
        pt[0] = pa[2 * (k + grids)];
        pt[1] = pa[2 * (k + grids) + 1];
    } else {
        const double lx = pa[2 * (N - 1)], ly = pa[2 * (N - 1) + 1];
        const double ex = lx - pa[2 * (N - 2)], ey = ly - pa[2 * (N - 2) + 1];
        const double m = (double)(k + 1) + ((double)grids - (double)N);
        pt[0] = lx + m * ex;
        pt[1] = ly + m * ey;
    }
}

// the disturbed plant (srb12_plant; compiled here, so that it shares the body above and this file's pragma)
#include "srb12_plant.hip"
