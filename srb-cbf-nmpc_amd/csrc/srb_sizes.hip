// Obstacle sizes (srb_sizes, DESIGN.md 3 "Obstacle sizes", 10.8): an optional CBF level (obs_eps, squared metres) and
// an optional body radius (obs_radius, metres) per obstacle row.  The solve kernels gather the level of each static
// column in their prologue (SRB_AGENT_OBSTACLES, srb_kernels.hip: eps[j] = obs_eps[sel[j]], the _mv_ instances); the
// device code of the rest of the feature is the four kernels here:
//   srb_knn_obs_clear_kernel            the K_obs rows of smallest clearance to their level set
//   srb_knn_obs_clear_scene_kernel      the same over the obstacle rows of the agent's scene
//   srb_sim_metrics_sized_kernel        srb_sim_metrics_kernel with d_obs = min_i (dist_i - obs_radius[i])
//   srb_sim_scene_metrics_sized_kernel  the same with blocks of one scene each
// The selection's order, tie, NaN and 1000 m rules are knn_insert / knn_pop's (srb_knn.h), the code of the snapshot
// selection, on a key that may be negative; the agent-to-agent half of the metrics is sim_nearest2 (srb_sim_scan.h).
// A translation unit of its own, as srb_scenes.hip and srb_moving.hip are and for their reason: every existing
// selection and metrics kernel keeps its machine code (tools/isa_diff.py).
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_wave.h"
#include "srb_knn.h"
#include "srb_sim_scan.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------- selection
// The agent's own points into LDS.  With a velocity table (srb_moving.horizon_selection = 1) the N + 1 points of
// srb_knn_obs_horizon_kernel, point k at time Ts k at constant velocity from x0 = [x, xdot, y, ydot]; without, the
// position now alone.
__device__ __forceinline__ void obs_clear_own(int tid, const double *__restrict__ x0, bool horizon, int N, double Ts,
                                              double *own)
{
    if (horizon) {
        if (tid <= N) {
            const double tk = Ts * (double)tid;
            own[2 * tid] = x0[0] + x0[1] * tk;
            own[2 * tid + 1] = x0[2] + x0[3] * tk;
        }
    } else if (tid == 0) {
        own[0] = x0[0];
        own[1] = x0[2];
    }
}

// The scan: the K rows of n_obs with the smallest key sqrt(m) - sqrt(obs_eps[i]), m the squared distance now
// (obs_vel null) or srb_knn_obs_horizon_kernel's min over k = 0 .. N of the squared distances.  The key can be
// negative (the agent inside the level set), so the lists are filtered on the key itself, not on its square: a row
// enters a thread's list when its key is at most the list's K-th.  A NaN key -- a NaN row, a NaN or negative
// obs_eps -- fails that test and is never selected.  knn_pop merges the lists into sel[0..K) with the static
// table's 1000 m rule (cap = 1: a key >= 1000, or no row left, gives row 0).
template <int KM>
__device__ __forceinline__ void knn_obs_clear_select(int tid, const double *own, const double *__restrict__ obstacles,
                                                     const double *__restrict__ obs_vel,
                                                     const double *__restrict__ obs_eps, int n_obs, int N, double Ts,
                                                     int K, int *sel, double *wd_lds, int *wi_lds)
{
#pragma clang fp contract(off)
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { bd[j] = __builtin_inf(); bi[j] = 0x7fffffff; }
    double kth = __builtin_inf();                  // the K-th key of this thread's list
    for (int i = tid; i < n_obs; i += 64 * SRB_KNN_OBS_WAVES) {
        const double ox = obstacles[2 * (size_t)i], oy = obstacles[2 * (size_t)i + 1];
        double m;
        if (obs_vel) {                             // a kernel argument: uniform
            const double wx = obs_vel[2 * (size_t)i], wy = obs_vel[2 * (size_t)i + 1];
            m = __builtin_inf();
            for (int k = 0; k <= N; k++) {
                const double tk = Ts * (double)k;
                const double dx = own[2 * k] - (ox + wx * tk), dy = own[2 * k + 1] - (oy + wy * tk);
                const double d2 = dx * dx + dy * dy;
                m = (d2 < m || d2 != d2) ? d2 : m;   // the minimum; a NaN pair makes the key NaN for good
            }
        } else {
            const double dx = own[0] - ox, dy = own[1] - oy;
            m = dx * dx + dy * dy;
        }
        const double key = sqrt(m) - sqrt(obs_eps[i]);
        if (!(key <= kth)) continue;               // NaN keys fail: such rows are never selected
        knn_insert<KM>(bd, bi, key, i, K);
#pragma unroll
        for (int j = 0; j < KM; j++)
            if (j == K - 1) kth = bd[j];
    }
    knn_pop<SRB_KNN_OBS_WAVES, KM>(tid, bd, bi, K, 1, sel, wd_lds, wi_lds);
}

// One workgroup per agent, brute force over the whole table: no grid is built or consulted.  Only the static
// columns are written (sel_out rows of stride sel_stride, columns 0 .. K_obs - 1).
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_OBS_WAVES) srb_knn_obs_clear_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, const double *__restrict__ obs_vel,
                const double *__restrict__ obs_eps, int n_obs, int N, double Ts, int K_obs, int *__restrict__ sel_out,
                int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_OBS_WAVES];
    __shared__ int wi_lds[SRB_KNN_OBS_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    obs_clear_own(tid, x0g + 4 * (size_t)agent, obs_vel != nullptr, N, Ts, own);
    __syncthreads();
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_obs <= 4) knn_obs_clear_select<4>(tid, own, obstacles, obs_vel, obs_eps, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else if (K_obs <= 8) knn_obs_clear_select<8>(tid, own, obstacles, obs_vel, obs_eps, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else knn_obs_clear_select<SRB_KNN_MAX>(tid, own, obstacles, obs_vel, obs_eps, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
}

// The same key over rows [scene scene_obs, + scene_obs) of the tables, scene = (agent_offset + agent) / scene_agents;
// global indices out: each thread re-bases the entry it stored itself (knn_pop: threads tid < K), so the 1000 m
// rule's local row 0 becomes the scene's row 0.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_OBS_WAVES) srb_knn_obs_clear_scene_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, const double *__restrict__ obs_vel,
                const double *__restrict__ obs_eps, int N, double Ts, int agent_offset, int scene_agents, int scene_obs,
                int K_obs, int *__restrict__ sel_out, int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_OBS_WAVES];
    __shared__ int wi_lds[SRB_KNN_OBS_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    obs_clear_own(tid, x0g + 4 * (size_t)agent, obs_vel != nullptr, N, Ts, own);
    __syncthreads();
    const int ob0 = ((agent_offset + agent) / scene_agents) * scene_obs;
    const double *ob = obstacles + 2 * (size_t)ob0, *vl = obs_vel ? obs_vel + 2 * (size_t)ob0 : nullptr;
    const double *ep = obs_eps + (size_t)ob0;
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_obs <= 4) knn_obs_clear_select<4>(tid, own, ob, vl, ep, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else if (K_obs <= 8) knn_obs_clear_select<8>(tid, own, ob, vl, ep, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else knn_obs_clear_select<SRB_KNN_MAX>(tid, own, ob, vl, ep, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    if (tid < K_obs) sel[tid] += ob0;              // (the static rule never leaves a -1)
}

// ---------------------------------------------------------------------------------------------- metrics
// (the clearance scan sim_clearance is in srb_sim_scan.h, shared with srb_agents.hip)

// agent a's metrics of cycle c from its smallest clearance to an obstacle body (cl_ob) and its smallest squared
// distance to another agent (b_ag): sim_metrics_store's rules with d_obs = cl_ob and the fail test d_obs < 0
__device__ static __forceinline__ void sim_metrics_store_sized(int a, int c, int c_first, double px, double py,
                                                               double cl_ob, double b_ag, double *__restrict__ d_obs,
                                                               double *__restrict__ d_agent,
                                                               double *__restrict__ min_d_obs,
                                                               double *__restrict__ min_d_agent,
                                                               int *__restrict__ fail_cycle,
                                                               double *__restrict__ distance_to_fail)
{
#pragma clang fp contract(off)
    const double dob = cl_ob, dag = sqrt(b_ag);
    const bool first = c == c_first;
    if (d_obs) d_obs[a] = dob;
    if (d_agent) d_agent[a] = dag;
    if (min_d_obs) min_d_obs[a] = (first || dob < min_d_obs[a]) ? dob : min_d_obs[a];
    if (min_d_agent) min_d_agent[a] = (first || dag < min_d_agent[a]) ? dag : min_d_agent[a];
    if (fail_cycle) {
        int fc = first ? -1 : fail_cycle[a];
        if (first && distance_to_fail) distance_to_fail[a] = 0.0;
        if (fc < 0 && dob < 0.0) {
            fc = c;
            if (distance_to_fail) distance_to_fail[a] = sqrt(px * px + py * py);
        }
        fail_cycle[a] = fc;
    }
}

// srb_sim_metrics_kernel's geometry: SIM_AG agents per block of SIM_TILE threads, SIM_SL threads per agent
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_metrics_sized_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles,
    const double *__restrict__ obs_radius, int n_obs, const double *__restrict__ nbr_state, int n_all, int agent_offset,
    double *__restrict__ d_obs, double *__restrict__ d_agent, double *__restrict__ min_d_obs,
    double *__restrict__ min_d_agent, int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail)
{
    __shared__ double2 tile[SIM_TILE];
    __shared__ double rtile[SIM_TILE];
    __shared__ double part[2][SIM_SL][SIM_AG];
    const int al = (int)threadIdx.x % SIM_AG, slice = (int)threadIdx.x / SIM_AG;
    const int a = blockIdx.x * SIM_AG + al;
    const bool live = a < n_agents;
    const double px = live ? state[4 * (size_t)a] : 0.0, py = live ? state[4 * (size_t)a + 2] : 0.0;
    double b_ob = sim_clearance(obstacles, obs_radius, n_obs, px, py, tile, rtile);
    double b_ag = sim_nearest2(nbr_state, n_all, 4, agent_offset + a, px, py, tile);
    part[0][slice][al] = b_ob;
    part[1][slice][al] = b_ag;
    __syncthreads();
    if (!live || slice != 0) return;
    for (int s = 1; s < SIM_SL; s++) {
        if (part[0][s][al] < b_ob) b_ob = part[0][s][al];
        if (part[1][s][al] < b_ag) b_ag = part[1][s][al];
    }
    sim_metrics_store_sized(a, c, c_first, px, py, b_ob, b_ag, d_obs, d_agent, min_d_obs, min_d_agent, fail_cycle,
                            distance_to_fail);
}

// srb_sim_scene_metrics_kernel's geometry: block b the agents (b % blocks_per_scene) SIM_AG .. of scene
// scene0 + b / blocks_per_scene, staging only that scene's obs_rows / nbr_rows rows
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_scene_metrics_sized_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles,
    const double *__restrict__ obs_radius, int obs_rows, const double *__restrict__ nbr_state, int nbr_rows,
    int scene_agents, int agent_offset, int scene0, int blocks_per_scene, double *__restrict__ d_obs,
    double *__restrict__ d_agent, double *__restrict__ min_d_obs, double *__restrict__ min_d_agent,
    int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail)
{
    __shared__ double2 tile[SIM_TILE];
    __shared__ double rtile[SIM_TILE];
    __shared__ double part[2][SIM_SL][SIM_AG];
    const int al = (int)threadIdx.x % SIM_AG, slice = (int)threadIdx.x / SIM_AG;
    const int scene = scene0 + (int)blockIdx.x / blocks_per_scene;
    const int loc = ((int)blockIdx.x % blocks_per_scene) * SIM_AG + al;          // the agent's row of its scene
    const int a = scene * scene_agents + loc - agent_offset;                     // and of the batch
    const bool live = loc < scene_agents && a >= 0 && a < n_agents;
    const double px = live ? state[4 * (size_t)a] : 0.0, py = live ? state[4 * (size_t)a + 2] : 0.0;
    double b_ob = sim_clearance(obstacles + 2 * (size_t)scene * obs_rows, obs_radius + (size_t)scene * obs_rows, obs_rows,
                                px, py, tile, rtile);
    double b_ag = sim_nearest2(nbr_state + 4 * (size_t)scene * nbr_rows, nbr_rows, 4, loc, px, py, tile);
    part[0][slice][al] = b_ob;
    part[1][slice][al] = b_ag;
    __syncthreads();
    if (!live || slice != 0) return;
    for (int s = 1; s < SIM_SL; s++) {
        if (part[0][s][al] < b_ob) b_ob = part[0][s][al];
        if (part[1][s][al] < b_ag) b_ag = part[1][s][al];
    }
    sim_metrics_store_sized(a, c, c_first, px, py, b_ob, b_ag, d_obs, d_agent, min_d_obs, min_d_agent, fail_cycle,
                            distance_to_fail);
}
