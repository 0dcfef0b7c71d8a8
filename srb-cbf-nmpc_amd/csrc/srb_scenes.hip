// Scenes (srb_ctx_set_scenes): the batch as a set of independent teams.  Global agent
// g = agent_offset + agent belongs to scene g / scene_agents, whose tables are rows [scene scene_obs, + scene_obs)
// of obstacles and [scene scene_agents, + scene_agents) of nbr_state / nbr_plan.  "Which team is this agent in" is
// a matter for the selection and the safety metrics alone (the solve kernels read sel[j] as a global row), so the
// device code of the feature is the three kernels here:
//   srb_knn_scene_kernel          srb_knn_kernel on the scene's sub-tables
//   srb_knn_plan_scene_kernel     srb_knn_plan_kernel on the scene's rows
//   srb_sim_scene_metrics_kernel  srb_sim_metrics_kernel with blocks of one scene each
// Each hands the scene's sub-table (pointer, row count and self index scene-local, no grid) to the device functions
// of its unsegmented kernel -- knn_select / knn_plan_select (srb_knn.h), sim_nearest2 / sim_metrics_store
// (srb_sim_scan.h) -- so the order, tie, NaN, self, 1000 m and -1 rules and the distances are the same code.
// A translation unit of its own: added to srb_select.hip and srb_sim.hip, the kernels changed the instruction
// order of srb_knn_plan_kernel and srb_sim_metrics_kernel (tools/isa_diff.py), whatever their place in the file.
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_wave.h"
#include "srb_knn.h"
#include "srb_sim_scan.h"

#pragma clang fp contract(off)

// rows [0, K) of sel were stored by threads tid < K (knn_pop): each re-bases its own entry, the global sel row
// read back by the thread that wrote it (never an LDS pointer through knn_select's int *sel: a generic access)
__device__ __forceinline__ void knn_scene_rebase(int tid, int K, int base, int *sel)
{
    if (tid < K) {
        const int v = sel[tid];
        if (v >= 0) sel[tid] = v + base;           // -1 (no row) stays
    }
}

// One workgroup per agent, the two tables on the two waves as in srb_knn_kernel.  Scene tables are small (a team
// and its obstacles: a few rows a wave), so there is no grid; a single table of more than 64 SRB_KNN_RB rows a
// scene is scanned by both waves, as there.  The static 1000 m rule selects local row 0, the scene's row 0 after
// the re-base.  (Four agents per workgroup, one wave per agent doing its two tables in turn, measured slower at
// 8 agents + 20 obstacles a scene: selection 12.2 us against 9.4 us)
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_WAVES) srb_knn_scene_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, const double *__restrict__ nbr_state,
                int agent_offset, int scene_agents, int scene_obs, int K_obs, int K_nbr, int *__restrict__ sel_out,
                int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_WAVES];
    __shared__ int wi_lds[SRB_KNN_WAVES];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const double px = x0g[4 * (size_t)agent], py = x0g[4 * (size_t)agent + 2];
    const int g = agent_offset + agent, scene = g / scene_agents;
    const int ob0 = scene * scene_obs, nb0 = scene * scene_agents, self = g - nb0;
    const double *ob = obstacles + 2 * (size_t)ob0, *nb = nbr_state + 4 * (size_t)nb0;
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (SRB_KNN_WAVES == 2 && K_obs > 0 && K_nbr > 0) {
        const int lane = tid & 63;
        if (tid < 64) {
            knn_select<1>(lane, px, py, ob, 2, scene_obs, -1, K_obs, 1, sel, wd_lds, wi_lds);
            knn_scene_rebase(lane, K_obs, ob0, sel);
        } else {
            knn_select<1>(lane, px, py, nb, 4, scene_agents, self, K_nbr, 0, sel + K_obs, wd_lds, wi_lds);
            knn_scene_rebase(lane, K_nbr, nb0, sel + K_obs);
        }
        return;
    }
    if (SRB_KNN_WAVES == 2 && (K_obs > 0) != (K_nbr > 0)) {
        const bool o = K_obs > 0;
        if ((o ? scene_obs : scene_agents) <= 64 * SRB_KNN_RB) {
            if (tid >= 64) return;                     // whole wave: no barrier follows on the one-wave path
            if (o) {
                knn_select<1>(tid, px, py, ob, 2, scene_obs, -1, K_obs, 1, sel, wd_lds, wi_lds);
                knn_scene_rebase(tid, K_obs, ob0, sel);
            } else {
                knn_select<1>(tid, px, py, nb, 4, scene_agents, self, K_nbr, 0, sel + K_obs, wd_lds, wi_lds);
                knn_scene_rebase(tid, K_nbr, nb0, sel + K_obs);
            }
            return;
        }
    }
    if (K_obs > 0) {
        knn_select<SRB_KNN_WAVES>(tid, px, py, ob, 2, scene_obs, -1, K_obs, 1, sel, wd_lds, wi_lds);
        knn_scene_rebase(tid, K_obs, ob0, sel);
    }
    if (K_nbr > 0) {
        knn_select<SRB_KNN_WAVES>(tid, px, py, nb, 4, scene_agents, self, K_nbr, 0, sel + K_obs, wd_lds, wi_lds);
        knn_scene_rebase(tid, K_nbr, nb0, sel + K_obs);
    }
}

// The horizon-aware key of srb_knn_plan_kernel over the scene's rows only: own plan nbr_plan[g], rows nbr_plan[i]
// for i in the scene; global indices to the neighbour columns.  own_plan [n_agents][N][2] (null: none), indexed by
// the local agent, replaces nbr_plan[g] as the agent's own plan, as in srb_knn_plan_kernel.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_PLAN_WAVES) srb_knn_plan_scene_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ nbr_state,
                const double *__restrict__ nbr_plan, int N, int agent_offset, int scene_agents, int K_nbr,
                int *__restrict__ sel_out, int sel_stride, const double *__restrict__ own_plan)
{
    __shared__ double wd_lds[SRB_KNN_PLAN_WAVES];
    __shared__ int wi_lds[SRB_KNN_PLAN_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const int g = agent_offset + agent, nb0 = (g / scene_agents) * scene_agents, self = g - nb0;
    const double *op = own_plan ? own_plan + 2 * (size_t)agent * N : nbr_plan + 2 * (size_t)g * N;
    if (tid < 2) own[tid] = x0g[4 * (size_t)agent + 2 * tid];
    else if (tid < 2 * N + 2) own[tid] = op[tid - 2];
    __syncthreads();
    const double *nb = nbr_state + 4 * (size_t)nb0, *pl = nbr_plan + 2 * (size_t)nb0 * N;
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_nbr <= 4) knn_plan_select<4>(tid, own, nb, pl, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    else if (K_nbr <= 8) knn_plan_select<8>(tid, own, nb, pl, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    else knn_plan_select<SRB_KNN_MAX>(tid, own, nb, pl, scene_agents, N, self, K_nbr, sel, wd_lds, wi_lds);
    knn_scene_rebase(tid, K_nbr, nb0, sel);
}

// Nearest obstacle and nearest other agent within the agent's scene.  Sixteen consecutive agents of
// srb_sim_metrics_kernel may straddle scenes, so here every block serves agents of one scene -- block b the agents
// (b % blocks_per_scene) SIM_AG .. of scene scene0 + b / blocks_per_scene, scene0 the scene of the batch's first
// agent -- and stages only that scene's obs_rows / nbr_rows rows.  A shard may begin or end inside a scene: agents
// of the scene outside the batch are not live.  A minimum is exact in any order and the distances are the same
// expressions, so the bits equal a per-scene call of srb_sim_metrics_kernel.
extern "C" __global__ void __launch_bounds__(SIM_TILE) srb_sim_scene_metrics_kernel(
    int n_agents, int c, int c_first, const double *__restrict__ state, const double *__restrict__ obstacles,
    int obs_rows, const double *__restrict__ nbr_state, int nbr_rows, int scene_agents, int agent_offset, int scene0,
    int blocks_per_scene, double *__restrict__ d_obs, double *__restrict__ d_agent, double *__restrict__ min_d_obs,
    double *__restrict__ min_d_agent, int *__restrict__ fail_cycle, double *__restrict__ distance_to_fail)
{
    __shared__ double2 tile[SIM_TILE];
    __shared__ double part[2][SIM_SL][SIM_AG];
    const int al = (int)threadIdx.x % SIM_AG, slice = (int)threadIdx.x / SIM_AG;
    const int scene = scene0 + (int)blockIdx.x / blocks_per_scene;
    const int loc = ((int)blockIdx.x % blocks_per_scene) * SIM_AG + al;          // the agent's row of its scene
    const int a = scene * scene_agents + loc - agent_offset;                     // and of the batch
    const bool live = loc < scene_agents && a >= 0 && a < n_agents;
    const double px = live ? state[4 * (size_t)a] : 0.0, py = live ? state[4 * (size_t)a + 2] : 0.0;
    double b_ob = sim_nearest2(obstacles + 2 * (size_t)scene * obs_rows, obs_rows, 2, -1, px, py, tile);
    double b_ag = sim_nearest2(nbr_state + 4 * (size_t)scene * nbr_rows, nbr_rows, 4, loc, px, py, tile);
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
