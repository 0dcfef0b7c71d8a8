// Agent sizes (srb_agent_sizes, DESIGN.md 3 "Agent sizes", 10.10): an optional safety radius (agent_rad), pad
// (agent_pad) and body radius (agent_body) per row of the neighbour table.  The solve kernels rewrite the levels of
// their columns in their prologue (SRB_AGENT_OBSTACLES, srb_kernels.hip, the _mv_ instances); the device code of the
// rest of the feature is the four kernels here:
//   srb_knn_nbr_clear_kernel             the K_nbr rows of smallest clearance dist_i - agent_rad[i]
//   srb_knn_nbr_clear_scene_kernel       the same over the rows of the agent's scene
//   srb_sim_metrics_agents_kernel        the metrics with d_agent = min_i (dist_i - (body[g] + body[i])), collide_cycle
//   srb_sim_scene_metrics_agents_kernel  the same with blocks of one scene each
// The selection's order, tie, NaN and -1 rules are knn_insert / knn_pop's (srb_knn.h) on a key that may be negative,
// its distances those of srb_knn_kernel (the snapshot) or knn_plan_select (the horizon); the obstacle half of the
// metrics is sim_nearest2 or sim_clearance (srb_sim_scan.h).  A translation unit of its own, as srb_sizes.hip is and
// for its reason: every existing selection and metrics kernel keeps its machine code (tools/isa_diff.py).
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_wave.h"
#include "srb_knn.h"
#include "srb_sim_scan.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------- selection
// The agent's own points into LDS as srb_knn_plan_kernel lays them out: the snapshot position, then (with a plan
// table) the N points of its own plan row g.
__device__ __forceinline__ void nbr_clear_own(int tid, const double *__restrict__ x0, const double *__restrict__ nbr_plan,
                                              int g, int N, double *own)
{
    if (tid < 2) own[tid] = x0[2 * tid];
    else if (nbr_plan && tid < 2 * N + 2) own[tid] = nbr_plan[2 * (size_t)g * N + tid - 2];
}

// The scan: the K rows of n_all with the smallest key sqrt(m) - agent_rad[i], row `self` left out; m the squared
// snapshot distance (nbr_plan null) or knn_plan_select's minimum over the N + 1 pairs.  The agent's own radius would
// shift every key alike and is left out.  The key can be negative, so the lists are filtered on the key itself
// (knn_obs_clear_select's filter): a row enters a thread's list when its key is at most the list's K-th.  A NaN key
// -- a NaN row, a NaN radius -- fails that test and is never selected.  knn_pop merges the lists into sel[0..K)
// without the 1000 m rule (cap = 0: a slot with no row left gets -1).
template <int KM>
__device__ __forceinline__ void knn_nbr_clear_select(int tid, const double *own, const double *__restrict__ nbr_state,
                                                     const double *__restrict__ nbr_plan,
                                                     const double *__restrict__ agent_rad, int n_all, int N, int self,
                                                     int K, int *sel, double *wd_lds, int *wi_lds)
{
#pragma clang fp contract(off)
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { bd[j] = __builtin_inf(); bi[j] = 0x7fffffff; }
    double kth = __builtin_inf();                  // the K-th key of this thread's list
    for (int i = tid; i < n_all; i += 64 * SRB_KNN_PLAN_WAVES) {
        if (i == self) continue;
        const double dx0 = own[0] - nbr_state[4 * (size_t)i], dy0 = own[1] - nbr_state[4 * (size_t)i + 1];
        double m = dx0 * dx0 + dy0 * dy0;
        if (nbr_plan) {                            // a kernel argument: uniform
            const double *row = nbr_plan + 2 * (size_t)i * N;
            for (int k = 0; k < N; k++) {
                const double dx = own[2 * k + 2] - row[2 * k], dy = own[2 * k + 3] - row[2 * k + 1];
                const double d2 = dx * dx + dy * dy;
                m = (d2 < m || d2 != d2) ? d2 : m;   // the minimum; a NaN pair makes the key NaN for good
            }
        }
        const double key = sqrt(m) - agent_rad[i];
        if (!(key <= kth)) continue;               // NaN keys fail: such rows are never selected
        knn_insert<KM>(bd, bi, key, i, K);
#pragma unroll
        for (int j = 0; j < KM; j++)
            if (j == K - 1) kth = bd[j];
    }
    knn_pop<SRB_KNN_PLAN_WAVES, KM>(tid, bd, bi, K, 0, sel, wd_lds, wi_lds);
}

// One workgroup per agent, brute force over the whole table: no grid is built or consulted.  Only the neighbour
// columns are written (sel_out points at them; rows of stride sel_stride), srb_knn_plan_kernel's convention.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_PLAN_WAVES) srb_knn_nbr_clear_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ nbr_state,
                const double *__restrict__ nbr_plan, const double *__restrict__ agent_rad, int n_all, int N,
                int agent_offset, int K_nbr, int *__restrict__ sel_out, int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_PLAN_WAVES];
    __shared__ int wi_lds[SRB_KNN_PLAN_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const int g = agent_offset + agent;
    nbr_clear_own(tid, x0g + 4 * (size_t)agent, nbr_plan, g, N, own);
    __syncthreads();
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_nbr <= 4) knn_nbr_clear_select<4>(tid, own, nbr_state, nbr_plan, agent_rad, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
    else if (K_nbr <= 8) knn_nbr_clear_select<8>(tid, own, nbr_state, nbr_plan, agent_rad, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
    else knn_nbr_clear_select<SRB_KNN_MAX>(tid, own, nbr_state, nbr_plan, agent_rad, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
}

// The same key over rows [nb0, nb0 + scene_agents) of the tables, nb0 the first row of the agent's scene; global
// indices out: each thread re-bases the entry it stored itself (knn_pop: threads tid < K), as knn_scene_rebase of
// srb_scenes.hip does, and a -1 (no row left) stays.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_PLAN_WAVES) srb_knn_nbr_clear_scene_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ nbr_state,
                const double *__restrict__ nbr_plan, const double *__restrict__ agent_rad, int N, int agent_offset,
                int scene_agents, int K_nbr, int *__restrict__ sel_out, int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_PLAN_WAVES];
    __shared__ int wi_lds[SRB_KNN_PLAN_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const int g = agent_offset + agent, nb0 = (g / scene_agents) * scene_agents, self = g - nb0;
    nbr_clear_own(tid, x0g + 4 * (size_t)agent, nbr_plan, g, N, own);
    __syncthreads();
    const double *nb = nbr_state + 4 * (size_t)nb0, *pl = nbr_plan ? nbr_plan + 2 * (size_t)nb0 * N : nullptr;
    const double *rd = agent_rad + (size_t)nb0;
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_nbr <= 4) knn_nbr_clear_select<4>(tid, own, nb, pl, rd, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    else if (K_nbr <= 8) knn_nbr_clear_select<8>(tid, own, nb, pl, rd, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    else knn_nbr_clear_select<SRB_KNN_MAX>(tid, own, nb, pl, rd, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    if (tid < K_nbr) {
        const int v = sel[tid];
        if (v >= 0) sel[tid] = v + nb0;            // -1 (no row) stays
    }
}

// ---------------------------------------------------------------------------------------------- metrics
// this thread's share of the smallest body clearance sqrt(d2_i) - (own + body[i]) from (px, py) to the n rows of the
// neighbour table (stride 4), row `skip` left out; every d2 formed as sim_nearest2 forms it and staged through LDS
// in its tiles, the body radii in a tile beside (every thread of the block calls this).  The sum of the two radii is
// one rounded add.  A clearance that is NaN never compares smaller; without another row the result is +inf.
__device__ static __forceinline__ double sim_body_clearance(const double *__restrict__ tab,
                                                            const double *__restrict__ body, int n, int skip, double own,
                                                            double px, double py, double2 *tile, double *rtile)
{
#pragma clang fp contract(off)
    const int slice = (int)threadIdx.x / SIM_AG;
    double best = INFINITY;
    for (int t0 = 0; t0 < n; t0 += SIM_TILE) {
        const int row = t0 + (int)threadIdx.x;
        __syncthreads();                                  // the previous tile has been read
        if (row < n) {
            tile[threadIdx.x] = make_double2(tab[(size_t)row * 4], tab[(size_t)row * 4 + 1]);
            rtile[threadIdx.x] = body[row];
        }
        __syncthreads();
        const int m = n - t0 < SIM_TILE ? n - t0 : SIM_TILE;
        for (int i = slice; i < m; i += SIM_SL) {
            const double dx = px - tile[i].x, dy = py - tile[i].y;
            const double d2 = dx * dx + dy * dy;
            const double both = own + rtile[i];
            const double cl = sqrt(d2) - both;
            if (t0 + i != skip && cl < best) best = cl;
        }
    }
    return best;
}

// agent a's metrics of cycle c from its obstacle measure dob (a centre distance with the fail test dob < 0.5, or
// with sized = true a body clearance with the fail test dob < 0) and its smallest body clearance to another agent
// (dag): sim_metrics_store's rules, and collide_cycle by fail_cycle's (set at c == c_first, then the first cycle
// with dag < 0, never overwritten).  fail_cycle and distance_to_fail do not look at agent bodies.
__device__ static __forceinline__ void sim_metrics_store_agents(int a, int c, int c_first, double px, double py,
                                                                double dob, bool sized, double dag,
                                                                double *__restrict__ d_obs, double *__restrict__ d_agent,
                                                                double *__restrict__ min_d_obs,
                                                                double *__restrict__ min_d_agent,
                                                                int *__restrict__ fail_cycle,
                                                                double *__restrict__ distance_to_fail,
                                                                int *__restrict__ collide_cycle)
{
#pragma clang fp contract(off)
    const bool first = c == c_first;
    if (d_obs) d_obs[a] = dob;
    if (d_agent) d_agent[a] = dag;
    if (min_d_obs) min_d_obs[a] = (first || dob < min_d_obs[a]) ? dob : min_d_obs[a];
    if (min_d_agent) min_d_agent[a] = (first || dag < min_d_agent[a]) ? dag : min_d_agent[a];
    if (fail_cycle) {
        int fc = first ? -1 : fail_cycle[a];
        if (first && distance_to_fail) distance_to_fail[a] = 0.0;
        if (fc < 0 && dob < (sized ? 0.0 : 0.5)) {
            fc = c;
            if (distance_to_fail) distance_to_fail[a] = sqrt(px * px + py * py);
        }
        fail_cycle[a] = fc;
    }
    if (collide_cycle) {
        int cc = first ? -1 : collide_cycle[a];
        if (cc < 0 && dag < 0.0) cc = c;
        collide_cycle[a] = cc;
    }
}

// srb_sim_metrics_sized_kernel's geometry: SIM_AG agents per block of SIM_TILE threads, SIM_SL threads per agent.
// obs_radius null (a kernel argument: uniform, so are the barriers inside the scans): srb_sim's obstacle half.
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_metrics_agents_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles,
    const double *__restrict__ obs_radius, int n_obs, const double *__restrict__ nbr_state,
    const double *__restrict__ agent_body, int n_all, int agent_offset, double *__restrict__ d_obs,
    double *__restrict__ d_agent, double *__restrict__ min_d_obs, double *__restrict__ min_d_agent,
    int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail, int *__restrict__ collide_cycle)
{
    __shared__ double2 tile[SIM_TILE];
    __shared__ double rtile[SIM_TILE];
    __shared__ double part[2][SIM_SL][SIM_AG];
    const int al = (int)threadIdx.x % SIM_AG, slice = (int)threadIdx.x / SIM_AG;
    const int a = blockIdx.x * SIM_AG + al;
    const bool live = a < n_agents;
    const double px = live ? state[4 * (size_t)a] : 0.0, py = live ? state[4 * (size_t)a + 2] : 0.0;
    const double own = (live && n_all > 0) ? agent_body[(size_t)agent_offset + a] : 0.0;
    double b_ob = obs_radius ? sim_clearance(obstacles, obs_radius, n_obs, px, py, tile, rtile)
                             : sqrt(sim_nearest2(obstacles, n_obs, 2, -1, px, py, tile));
    double b_ag = sim_body_clearance(nbr_state, agent_body, n_all, agent_offset + a, own, px, py, tile, rtile);
    part[0][slice][al] = b_ob;
    part[1][slice][al] = b_ag;
    __syncthreads();
    if (!live || slice != 0) return;
    for (int s = 1; s < SIM_SL; s++) {
        if (part[0][s][al] < b_ob) b_ob = part[0][s][al];
        if (part[1][s][al] < b_ag) b_ag = part[1][s][al];
    }
    sim_metrics_store_agents(a, c, c_first, px, py, b_ob, obs_radius != nullptr, b_ag, d_obs, d_agent, min_d_obs,
                             min_d_agent, fail_cycle, distance_to_fail, collide_cycle);
}

// srb_sim_scene_metrics_sized_kernel's geometry: block b the agents (b % blocks_per_scene) SIM_AG .. of scene
// scene0 + b / blocks_per_scene, staging only that scene's obs_rows / nbr_rows rows
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_scene_metrics_agents_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles,
    const double *__restrict__ obs_radius, int obs_rows, const double *__restrict__ nbr_state,
    const double *__restrict__ agent_body, int nbr_rows, int scene_agents, int agent_offset, int scene0,
    int blocks_per_scene, double *__restrict__ d_obs, double *__restrict__ d_agent, double *__restrict__ min_d_obs,
    double *__restrict__ min_d_agent, int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail,
    int *__restrict__ collide_cycle)
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
    const double *body = agent_body + (size_t)scene * nbr_rows;
    const double own = (live && nbr_rows > 0) ? body[loc] : 0.0;
    const double *ob = obstacles + 2 * (size_t)scene * obs_rows;
    double b_ob = obs_radius ? sim_clearance(ob, obs_radius + (size_t)scene * obs_rows, obs_rows, px, py, tile, rtile)
                             : sqrt(sim_nearest2(ob, obs_rows, 2, -1, px, py, tile));
    double b_ag = sim_body_clearance(nbr_state + 4 * (size_t)scene * nbr_rows, body, nbr_rows, loc, own, px, py, tile,
                                     rtile);
    part[0][slice][al] = b_ob;
    part[1][slice][al] = b_ag;
    __syncthreads();
    if (!live || slice != 0) return;
    for (int s = 1; s < SIM_SL; s++) {
        if (part[0][s][al] < b_ob) b_ob = part[0][s][al];
        if (part[1][s][al] < b_ag) b_ag = part[1][s][al];
    }
    sim_metrics_store_agents(a, c, c_first, px, py, b_ob, obs_radius != nullptr, b_ag, d_obs, d_agent, min_d_obs,
                             min_d_agent, fail_cycle, distance_to_fail, collide_cycle);
}
