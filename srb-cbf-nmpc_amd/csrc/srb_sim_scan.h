// The tiled nearest-row scan of the rollout's safety metrics, shared by srb_sim_metrics_kernel (srb_sim.hip) and its
// per-scene form (srb_scenes.hip), and the clearance scan of the sized metrics (srb_sizes.hip, srb_agents.hip).
// Header-only, device code; fp64 with contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include "srb_kernel_decls.h"

#define SIM_TILE 256
#define SIM_AG SRB_SIM_AGENTS_PER_BLOCK            // agents per block
#define SIM_SL (SIM_TILE / SIM_AG)                 // threads per agent: each scans every SIM_SL-th row of a tile

// this thread's share of the smallest squared distance from (px, py) to the rows of tab (row stride `stride`
// doubles, columns 0 and 1), row `skip` left out.  The block stages the rows through LDS in tiles of SIM_TILE and
// thread (agent, slice) scans rows slice, slice + SIM_SL, .. of each tile, so every thread of the block calls this
// (threads past the batch's end included).  A squared distance that is NaN never compares smaller.
__device__ static __forceinline__ double sim_nearest2(const double *__restrict__ tab, int n, int stride, int skip,
                                                      double px, double py, double2 *tile)
{
#pragma clang fp contract(off)
    const int slice = (int)threadIdx.x / SIM_AG;
    double best = INFINITY;
    for (int t0 = 0; t0 < n; t0 += SIM_TILE) {
        const int row = t0 + (int)threadIdx.x;
        __syncthreads();                                  // the previous tile has been read
        if (row < n) tile[threadIdx.x] = make_double2(tab[(size_t)row * stride], tab[(size_t)row * stride + 1]);
        __syncthreads();
        const int m = n - t0 < SIM_TILE ? n - t0 : SIM_TILE;
        for (int i = slice; i < m; i += SIM_SL) {
            const double dx = px - tile[i].x, dy = py - tile[i].y;
            const double d2 = dx * dx + dy * dy;
            if (t0 + i != skip && d2 < best) best = d2;
        }
    }
    return best;
}

// this thread's share of the smallest clearance sqrt(d2_i) - rad[i] from (px, py) to the n obstacle rows, every d2
// formed as sim_nearest2 forms it and staged through LDS in its tiles (every thread of the block calls this).  A
// clearance that is NaN never compares smaller; without a row the result is +inf.
__device__ static __forceinline__ double sim_clearance(const double *__restrict__ tab, const double *__restrict__ rad,
                                                       int n, double px, double py, double2 *tile, double *rtile)
{
#pragma clang fp contract(off)
    const int slice = (int)threadIdx.x / SIM_AG;
    double best = INFINITY;
    for (int t0 = 0; t0 < n; t0 += SIM_TILE) {
        const int row = t0 + (int)threadIdx.x;
        __syncthreads();                                  // the previous tile has been read
        if (row < n) {
            tile[threadIdx.x] = make_double2(tab[(size_t)row * 2], tab[(size_t)row * 2 + 1]);
            rtile[threadIdx.x] = rad[row];
        }
        __syncthreads();
        const int m = n - t0 < SIM_TILE ? n - t0 : SIM_TILE;
        for (int i = slice; i < m; i += SIM_SL) {
            const double dx = px - tile[i].x, dy = py - tile[i].y;
            const double d2 = dx * dx + dy * dy;
            const double cl = sqrt(d2) - rtile[i];
            if (cl < best) best = cl;
        }
    }
    return best;
}

// agent a's metrics of cycle c from its smallest squared distances (b_ob to an obstacle, b_ag to another agent)
__device__ static __forceinline__ void sim_metrics_store(int a, int c, int c_first, double px, double py, double b_ob,
                                                         double b_ag, double *__restrict__ d_obs,
                                                         double *__restrict__ d_agent, double *__restrict__ min_d_obs,
                                                         double *__restrict__ min_d_agent, int *__restrict__ fail_cycle,
                                                         double *__restrict__ distance_to_fail)
{
#pragma clang fp contract(off)
    const double dob = sqrt(b_ob), dag = sqrt(b_ag);
    const bool first = c == c_first;
    if (d_obs) d_obs[a] = dob;
    if (d_agent) d_agent[a] = dag;
    if (min_d_obs) min_d_obs[a] = (first || dob < min_d_obs[a]) ? dob : min_d_obs[a];
    if (min_d_agent) min_d_agent[a] = (first || dag < min_d_agent[a]) ? dag : min_d_agent[a];
    // updateDistance_to_fail (MPC_dist.cpp:21-40): the first cycle inside 0.5 m of an obstacle, and the distance
    // from the origin there; once set they stay (isSuccess)
    if (fail_cycle) {
        int fc = first ? -1 : fail_cycle[a];
        if (first && distance_to_fail) distance_to_fail[a] = 0.0;
        if (fc < 0 && dob < 0.5) {
            fc = c;
            if (distance_to_fail) distance_to_fail[a] = sqrt(px * px + py * py);
        }
        fail_cycle[a] = fc;
    }
}
