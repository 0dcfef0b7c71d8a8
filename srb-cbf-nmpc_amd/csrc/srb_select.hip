// Obstacle / neighbour selection kernels of the NMPC launch (srb_capi.cpp launch_select; shared with the SRB-12 mode).
// Included by srb_kernels.hip (part 0), see the note there; not a Makefile source of its own.
#include <hip/hip_runtime.h>
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_wave.h"
#include "srb_knn.h"

// Obstacle and neighbour selection (MPC_dist.cpp:371-396, generalised to K): one workgroup per
// agent, the K_obs nearest static obstacles (with the reference's 1000 m sentinel) and the
// K_nbr nearest other agents to the agent's own CoM, indices to sel_out[agent][K_obs + K_nbr]
// (-1: no neighbour row).  A kernel of its own rather than a phase of the solve: there the
// scan ran at the solve kernel's occupancy, one or two waves per CU, and took a quarter of
// the solve (profiles/r01_c3_stamps.txt).  Tables of SRB_GRID_MIN_ROWS rows or more come with
// a uniform grid (srb_grid_build_kernel) and only the cells around the agent are scanned.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_WAVES) srb_knn_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ obstacles, int n_obs,
                const double *__restrict__ nbr_state, int n_all, int agent_offset, int K_obs, int K_nbr,
                int *__restrict__ sel_out, int sel_stride, const SrbGrid *__restrict__ gob, const int *__restrict__ oob,
                const double2 *__restrict__ pob, const int *__restrict__ iob, const SrbGrid *__restrict__ gnb,
                const int *__restrict__ onb, const double2 *__restrict__ pnb, const int *__restrict__ inb)
{
    __shared__ double wd_lds[SRB_KNN_WAVES];
    __shared__ int wi_lds[SRB_KNN_WAVES];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const double px = x0g[4 * (size_t)agent], py = x0g[4 * (size_t)agent + 2];
    // sel_stride = Ko + Kn of the whole selection; a pass over one table (srb_select_device) hands over
    // K_obs or K_nbr alone and sel_out already offset to its columns
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (SRB_KNN_WAVES == 2 && K_obs > 0 && K_nbr > 0) {
        // the two tables on the two waves at once, each selection wave-local (DPP argmins, no barrier):
        // configs[2] selection 23.5 -> 20.9 us a step (HIP events, round 5; round 6's thresholded scan and ballot
        // argmin in srb_wave.h: 20.5 -> 13.4 us); the same rows.  (Selecting
        // inside the solve kernel's setup instead measured no faster at configs[2] -- the solve kernel
        // grew by what the launch saved -- and 4.6 % slower at N = 20, where four rounds of agents each
        // wait for their selection; round 5)
        const int lane = tid & 63;
        if (tid < 64)
            knn_select<1>(lane, px, py, obstacles, 2, n_obs, -1, K_obs, 1, sel, wd_lds, wi_lds, gob, oob, pob, iob);
        else
            knn_select<1>(lane, px, py, nbr_state, 4, n_all, agent_offset + agent, K_nbr, 0, sel + K_obs, wd_lds, wi_lds,
                          gnb, onb, pnb, inb);
        return;
    }
    // one table (srb_select_device's passes, or a batch without neighbour rows): a table that one wave scans
    // with the threshold pass (knn_thresh) or through a grid runs on wave 0 alone -- the two-wave form pays two
    // barriers per pop round (round 6: the neighbour pass of the multi-GPU step 19.3 us with both waves)
    if (SRB_KNN_WAVES == 2 && (K_obs > 0) != (K_nbr > 0)) {
        const bool o = K_obs > 0;
        const SrbGrid *g = o ? gob : gnb;
        if ((o ? n_obs : n_all) <= 64 * SRB_KNN_RB || (g && g->ok)) {
            if (tid >= 64) return;                     // whole wave: no barrier follows on the one-wave path
            if (o) knn_select<1>(tid, px, py, obstacles, 2, n_obs, -1, K_obs, 1, sel, wd_lds, wi_lds, gob, oob, pob, iob);
            else knn_select<1>(tid, px, py, nbr_state, 4, n_all, agent_offset + agent, K_nbr, 0, sel + K_obs, wd_lds, wi_lds,
                               gnb, onb, pnb, inb);
            return;
        }
    }
    if (K_obs > 0)
        knn_select<SRB_KNN_WAVES>(tid, px, py, obstacles, 2, n_obs, -1, K_obs, 1, sel, wd_lds, wi_lds, gob, oob, pob, iob);
    if (K_nbr > 0)
        knn_select<SRB_KNN_WAVES>(tid, px, py, nbr_state, 4, n_all, agent_offset + agent, K_nbr, 0, sel + K_obs, wd_lds,
                                  wi_lds, gnb, onb, pnb, inb);
}

// Horizon-aware neighbour selection (SRB_OPT_PLAN_SELECTION = 1): the K_nbr table rows of closest predicted
// approach to global agent g = agent_offset + agent.  The key of row i is sqrt(min_k d_k^2) over the N + 1 pairs
// k = 0 the snapshot (x0 against nbr_state[i].xy) and k >= 1 the plans nbr_plan[g][k-1] against nbr_plan[i][k-1];
// order, ties, the excluded row g, NaN rows and the -1 fill are knn_select_k's (no 1000 m cap: that rule is the
// static table's).  Brute force, one workgroup per agent: the agent's own N + 1 points in LDS, every thread scans
// rows tid, tid + 64 KW, .. and keeps a sorted list (knn_insert); knn_pop merges them.  Only the neighbour
// columns are written (sel_out points at them; rows of stride sel_stride).  The scan itself is knn_plan_select
// (srb_knn.h), shared with the per-scene kernel of srb_scenes.hip.  own_plan [n_agents][N][2] (null: none), indexed
// by the local agent: the agent's own N plan points come from own_plan[agent] instead of nbr_plan[g] -- under a
// degraded link (srb_link) the table is what the agent perceives of the others, and its row g a stale, noisy copy
// of a plan the agent knows exactly.  Still one stage of 2 N + 2 doubles per workgroup (the row's base pointer is
// chosen before the load); the keys of every other row come from nbr_state / nbr_plan and row g stays left out.
extern "C" __global__ void __launch_bounds__(64 * SRB_KNN_PLAN_WAVES) srb_knn_plan_kernel(int n_agents,
                const double *__restrict__ x0g, const double *__restrict__ nbr_state,
                const double *__restrict__ nbr_plan, int n_all, int N, int agent_offset, int K_nbr,
                int *__restrict__ sel_out, int sel_stride, const double *__restrict__ own_plan)
{
    __shared__ double wd_lds[SRB_KNN_PLAN_WAVES];
    __shared__ int wi_lds[SRB_KNN_PLAN_WAVES];
    __shared__ double own[2 * (SRB_MAX_N + 1)];
    const int agent = xcd_agent(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (agent >= n_agents) return;                 // whole workgroup: the barriers stay uniform
    const int g = agent_offset + agent;
    const double *op = own_plan ? own_plan + 2 * (size_t)agent * N : nbr_plan + 2 * (size_t)g * N;
    if (tid < 2) own[tid] = x0g[4 * (size_t)agent + 2 * tid];
    else if (tid < 2 * N + 2) own[tid] = op[tid - 2];
    __syncthreads();
    int *sel = sel_out + (size_t)agent * sel_stride;
    if (K_nbr <= 4) knn_plan_select<4>(tid, own, nbr_state, nbr_plan, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
    else if (K_nbr <= 8) knn_plan_select<8>(tid, own, nbr_state, nbr_plan, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
    else knn_plan_select<SRB_KNN_MAX>(tid, own, nbr_state, nbr_plan, n_all, N, g, K_nbr, sel, wd_lds, wi_lds);
}

// Uniform grid over one table per workgroup (block 0: table 0, block 1: table 1), rebuilt every
// launch (the neighbour snapshot moves every cycle): bounds of the finite rows, about two rows
// per cell (at most SRB_GRID_CELLS cells), counts by LDS atomics, one exclusive scan, scatter of
// the rows into cell order.  One workgroup of 1024 threads per table: a few microseconds for the
// tens of thousands of rows of an 8-GPU swarm, against a brute-force scan per agent.
__device__ __forceinline__ int grid_cell(double x, double y, double x0, double y0, double inv_h, int nx, int ny)
{
    const int cx = min(max((int)((x - x0) * inv_h), 0), nx - 1);
    const int cy = min(max((int)((y - y0) * inv_h), 0), ny - 1);
    return cy * nx + cx;
}

extern "C" __global__ void __launch_bounds__(1024) srb_grid_build_kernel(
    const double *__restrict__ tab0, int stride0, int n0, SrbGrid *g0, int *off0, double2 *spos0, int *sidx0,
    const double *__restrict__ tab1, int stride1, int n1, SrbGrid *g1, int *off1, double2 *spos1, int *sidx1)
{
    __shared__ int cnt[SRB_GRID_CELLS];
    __shared__ double red[4][16];
    __shared__ int part[1024];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *tab = blockIdx.x ? tab1 : tab0;
    const int stride = blockIdx.x ? stride1 : stride0, n = blockIdx.x ? n1 : n0;
    SrbGrid *g = blockIdx.x ? g1 : g0;
    int *off = blockIdx.x ? off1 : off0;
    double2 *spos = blockIdx.x ? spos1 : spos0;
    int *sidx = blockIdx.x ? sidx1 : sidx0;
    if (!g) return;
    // bounds of the finite rows
    double mnx = __builtin_inf(), mny = __builtin_inf(), mxx = -__builtin_inf(), mxy = -__builtin_inf();
    for (int i = tid; i < n; i += 1024) {
        const double x = tab[(size_t)stride * i], y = tab[(size_t)stride * i + 1];
        if (isfinite(x) && isfinite(y)) { mnx = fmin(mnx, x); mny = fmin(mny, y); mxx = fmax(mxx, x); mxy = fmax(mxy, y); }
    }
    mnx = wmin(mnx); mny = wmin(mny); mxx = wmax(mxx); mxy = wmax(mxy);
    if (lane == 0) { red[0][wv] = mnx; red[1][wv] = mny; red[2][wv] = mxx; red[3][wv] = mxy; }
    __syncthreads();
    mnx = red[0][0]; mny = red[1][0]; mxx = red[2][0]; mxy = red[3][0];
    for (int w = 1; w < 16; w++) {
        mnx = fmin(mnx, red[0][w]); mny = fmin(mny, red[1][w]); mxx = fmax(mxx, red[2][w]); mxy = fmax(mxy, red[3][w]);
    }
    if (!(mnx <= mxx)) {                           // no finite row: selection falls back to the scan
        if (tid == 0) g->ok = 0;
        return;
    }
    const double W = mxx - mnx, H = mxy - mny;
    const int target = min(max(n / 2, 1), SRB_GRID_CELLS);
    double h = sqrt(fmax(W * H, 1e-300) / target);
    if (!(h > 0.0) || !isfinite(h)) h = 1.0;
    h = fmax(h, fmax(W, H) / 4096.0);             // keeps nx, ny in range
    int nx = (int)(W / h) + 1, ny = (int)(H / h) + 1;
    while ((long long)nx * ny > SRB_GRID_CELLS) { h *= 1.25; nx = (int)(W / h) + 1; ny = (int)(H / h) + 1; }
    const double inv_h = 1.0 / h;
    const int C = nx * ny;
    for (int c = tid; c < C; c += 1024) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const double x = tab[(size_t)stride * i], y = tab[(size_t)stride * i + 1];
        if (isfinite(x) && isfinite(y)) atomicAdd(&cnt[grid_cell(x, y, mnx, mny, inv_h, nx, ny)], 1);
    }
    __syncthreads();
    // exclusive scan: per-thread chunk sums, a scan of the 1024 partials, chunk-local offsets
    const int chunk = (C + 1023) / 1024, c0 = tid * chunk, c1 = min(c0 + chunk, C);
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += cnt[c];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = (tid >= o) ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;                     // exclusive prefix of this chunk
    for (int c = c0; c < c1; c++) { const int v = cnt[c]; cnt[c] = run; off[c] = run; run += v; }
    if (tid == 1023) off[C] = part[1023];
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const double x = tab[(size_t)stride * i], y = tab[(size_t)stride * i + 1];
        if (isfinite(x) && isfinite(y)) {
            const int at = atomicAdd(&cnt[grid_cell(x, y, mnx, mny, inv_h, nx, ny)], 1);
            spos[at] = make_double2(x, y);
            sidx[at] = i;
        }
    }
    if (tid == 0) {
        SrbGrid r;
        r.x0 = mnx; r.y0 = mny; r.inv_h = inv_h; r.h = h; r.nx = nx; r.ny = ny; r.n = part[1023]; r.ok = 1;
        *g = r;
    }
}
