// Moving obstacles (srb_moving, DESIGN.md 3 "Moving obstacles", 10.6): an optional velocity row per obstacle.  The
// solve kernels read it in their prologue (SRB_AGENT_OBSTACLES, srb_kernels.hip: the static row of grid k at
// o + w Ts (k + 1)); the device code of the rest of the feature is the three kernels here:
//   srb_knn_obs_horizon_kernel        the K_obs rows of closest predicted approach over the horizon
//   srb_knn_obs_horizon_scene_kernel  the same over the obstacle rows of the agent's scene
//   srb_obstacles_advance_kernel      one control cycle of the table
// The scan is knn_obs_horizon_select (srb_knn.h), whose order, tie, NaN and 1000 m rules are knn_insert / knn_pop's:
// the code of the snapshot selection.  A translation unit of its own, as srb_scenes.hip is and for its reason:
// every existing kernel keeps its machine code (tools/isa_diff.py).
#include <hip/hip_runtime.h>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_wave.h"
#include "srb_knn.h"

#pragma clang fp contract(off)

// the agent's own N + 1 points into LDS: point k at time Ts k, constant velocity from x0 = [x, xdot, y, ydot] --
// also when the solve reads a plan table (the key needs no plan of the agent's own)
__device__ __forceinline__ void obs_horizon_own(int tid, const double *__restrict__ x0, int N, double Ts, double *own)
{
    if (tid <= N) {
        const double tk = Ts * (double)tid;
        own[2 * tid] = x0[0] + x0[1] * tk;
        own[2 * tid + 1] = x0[2] + x0[3] * tk;
    }
}

// One workgroup per agent, brute force over the whole table: no grid is built or consulted.  Only the static
// columns are written (sel_out rows of stride sel_stride, columns 0 .. K_obs - 1).
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_OBS_WAVES) srb_knn_obs_horizon_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, const double *__restrict__ obs_vel,
                int n_obs, int N, double Ts, int K_obs, int *__restrict__ sel_out, int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_OBS_WAVES];
    __shared__ int wi_lds[SRB_KNN_OBS_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    obs_horizon_own(tid, x0g + 4 * (size_t)agent, N, Ts, own);
    __syncthreads();
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_obs <= 4) knn_obs_horizon_select<4>(tid, own, obstacles, obs_vel, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else if (K_obs <= 8) knn_obs_horizon_select<8>(tid, own, obstacles, obs_vel, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else knn_obs_horizon_select<SRB_KNN_MAX>(tid, own, obstacles, obs_vel, n_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
}

// The same key over rows [scene scene_obs, + scene_obs) of both tables, scene = (agent_offset + agent) / scene_agents;
// global indices out: each thread re-bases the entry it stored itself (knn_pop: threads tid < K), so the 1000 m
// rule's local row 0 becomes the scene's row 0.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_OBS_WAVES) srb_knn_obs_horizon_scene_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, const double *__restrict__ obs_vel,
                int N, double Ts, int agent_offset, int scene_agents, int scene_obs, int K_obs,
                int *__restrict__ sel_out, int sel_stride)
{
    __shared__ double wd_lds[SRB_KNN_OBS_WAVES];
    __shared__ int wi_lds[SRB_KNN_OBS_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    obs_horizon_own(tid, x0g + 4 * (size_t)agent, N, Ts, own);
    __syncthreads();
    const int ob0 = ((agent_offset + agent) / scene_agents) * scene_obs;
    const double *ob = obstacles + 2 * (size_t)ob0, *vl = obs_vel + 2 * (size_t)ob0;
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_obs <= 4) knn_obs_horizon_select<4>(tid, own, ob, vl, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else if (K_obs <= 8) knn_obs_horizon_select<8>(tid, own, ob, vl, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    else knn_obs_horizon_select<SRB_KNN_MAX>(tid, own, ob, vl, scene_obs, N, Ts, K_obs, sel, wd_lds, wi_lds);
    if (tid < K_obs) sel[tid] += ob0;              // (the static rule never leaves a -1)
}

// One control cycle (NDOMAIN = 4 grids) of the obstacle table, one thread per row; no bounce, no interaction.
extern "C" __global__ void __launch_bounds__(256) srb_obstacles_advance_kernel(int n_obs, double Ts, double *obstacles,
                                                                               const double *__restrict__ obs_vel)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obs) return;
    const double step = Ts * 4.0;
    obstacles[2 * (size_t)i] = obstacles[2 * (size_t)i] + obs_vel[2 * (size_t)i] * step;
    obstacles[2 * (size_t)i + 1] = obstacles[2 * (size_t)i + 1] + obs_vel[2 * (size_t)i + 1] * step;
}
