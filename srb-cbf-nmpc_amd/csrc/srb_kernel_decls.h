// What the host launch code and the device code must agree on, defined once: the structs passed to kernels by
// value or by pointer, and the prototype of every extern "C" kernel.  Included by the .hip file that defines a
// kernel and by the C-ABI file that launches it, so a parameter list that drifts is a conflicting declaration at
// compile time instead of undefined behaviour at launch.
#pragma once
#include <hip/hip_runtime.h>
#include "srb_kernel_params.h"

// device pointers of one low-level batch (srb_ll_io order; srb_ll_capi.cpp to_dev, srb_llctrl.hip)
struct SrbLLDev {
    const int *ind;
    const double *q, *dq, *Dinv, *B, *Hv, *Jc, *dJc, *Js, *Jtoe, *Jhip, *toePos, *hipPos, *H0, *dH0, *y, *dy, *hd,
        *dhd, *fDes;
    double *tau, *QP_force, *ddq, *dq_out, *q_out, *V, *dV, *x;
    int *status, *iters;
};

// Uniform grid over the rows of a table (SURVEY 8(a) row a10 at swarm scale): built on the
// device each launch by srb_grid_build_kernel for tables of SRB_GRID_MIN_ROWS rows or more.
// Cells row-major (cy * nx + cx), rows of finite coordinates sorted by cell (the order inside
// a cell is arbitrary -- the selection order of srb_knn.h is exact whatever it is).
struct SrbGrid {
    double x0, y0, inv_h, h;       // origin and cell size
    int nx, ny, n;                 // cells per axis, rows in the grid
    int ok;                        // 0: not built (brute-force scan)
};

// ---- srb_kernels.hip: the solve kernel (INFIX empty, or f32_ for the fp32-factor instances) and the polish kernel;
// the instances that take table extras (mv_: further arguments, the velocity table of srb_moving, the level table
// of srb_sizes and the safety-radius and pad tables of srb_agent_sizes, each may be null; the polish kernel also the
// agent_offset that the agent tables' own row needs) of each
#define SRB_DECL_NMPC_(INFIX, NZL, TS, NW, NC, CC, KC)                                                         \
    extern "C" __global__ void srb_nmpc_kernel_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(               \
        SrbKParams prm, int n_agents, const double *x0g, const double *refg, const double *footg,              \
        const double *obstacles, int n_obs, const double *nbr_state, int n_all, int agent_offset,              \
        double *x_qp_out, double *x_out, double *obj_out, int *status_out, int *iters_out,                    \
        const double *alpha_buf, double *alpha_out, const int *sel_g, float *zpol_g, int zstride,             \
        const double *nbr_plan, double *plan_out);                                                            \
    extern "C" __global__ void srb_nmpc_kernel_mv_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(            \
        SrbKParams prm, int n_agents, const double *x0g, const double *refg, const double *footg,              \
        const double *obstacles, int n_obs, const double *nbr_state, int n_all, int agent_offset,              \
        double *x_qp_out, double *x_out, double *obj_out, int *status_out, int *iters_out,                    \
        const double *alpha_buf, double *alpha_out, const int *sel_g, float *zpol_g, int zstride,             \
        const double *nbr_plan, double *plan_out, const double *obs_vel, const double *obs_eps,               \
        const double *agent_rad, const double *agent_pad);
#define SRB_DECL_POLISH(NZL, TS, NW, NC, CC, KC)                                                              \
    extern "C" __global__ void srb_polish_kernel_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                   \
        SrbKParams prm, int n_agents, const double *x0g, const double *refg, const double *footg,              \
        const double *obstacles, const double *nbr_state, double *x_out, double *obj_out, int *status_out,     \
        const double *alpha_buf, double *alpha_out, const int *sel_g, const float *zpol_g, int zstride,       \
        const double *nbr_plan, double *plan_out);                                                            \
    extern "C" __global__ void srb_polish_kernel_mv_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                \
        SrbKParams prm, int n_agents, const double *x0g, const double *refg, const double *footg,              \
        const double *obstacles, const double *nbr_state, double *x_out, double *obj_out, int *status_out,     \
        const double *alpha_buf, double *alpha_out, const int *sel_g, const float *zpol_g, int zstride,       \
        const double *nbr_plan, double *plan_out, const double *obs_vel, const double *obs_eps,               \
        const double *agent_rad, const double *agent_pad, int agent_offset);
#define SRB_DECL_NMPC(...) SRB_DECL_NMPC_(, __VA_ARGS__) SRB_DECL_POLISH(__VA_ARGS__)
#define SRB_DECL_NMPC_F32(...) SRB_DECL_NMPC_(f32_, __VA_ARGS__)
SRB_KERNEL_INSTANCES(SRB_DECL_NMPC)
#ifndef SRB_DEV_INSTANCES
SRB_KF32_INSTANCES(SRB_DECL_NMPC_F32)
#endif
#undef SRB_DECL_NMPC_
#undef SRB_DECL_POLISH
#undef SRB_DECL_NMPC
#undef SRB_DECL_NMPC_F32

// ---- srb_select.hip (compiled as part of srb_kernels.hip)
extern "C" __global__ void srb_knn_kernel(int n_agents, const double *x0g, const double *obstacles, int n_obs,
                                          const double *nbr_state, int n_all, int agent_offset, int K_obs, int K_nbr,
                                          int *sel_out, int sel_stride, const SrbGrid *gob, const int *oob, const double2 *pob,
                                          const int *iob, const SrbGrid *gnb, const int *onb, const double2 *pnb,
                                          const int *inb);
extern "C" __global__ void srb_knn_plan_kernel(int n_agents, const double *x0g, const double *nbr_state,
                                               const double *nbr_plan, int n_all, int N, int agent_offset, int K_nbr,
                                               int *sel_out, int sel_stride, const double *own_plan);
extern "C" __global__ void srb_grid_build_kernel(const double *tab0, int stride0, int n0, SrbGrid *g0, int *off0,
                                                 double2 *spos0, int *sidx0, const double *tab1, int stride1, int n1,
                                                 SrbGrid *g1, int *off1, double2 *spos1, int *sidx1);

// ---- srb_prepare.hip, srb_hlplan.hip
extern "C" __global__ void srb_prepare_kernel(int n_agents, int N, int C, int n_rows, int T, int agent_offset,
                                              const double *Pr, const double *Prd, const int *agent_id,
                                              const int *gait_domain, const int *contact, const double *toe,
                                              const double *start, const double *q, const double *dq, double *x0,
                                              double *ref, double *foot, double *last_state, int *status);
extern "C" __global__ void srb_hlplan_kernel(int NA, const double *Pstart, const double *Pobs, int n_obs, int loop,
                                             double *Pr, double *Prd);
extern "C" __global__ void srb_hlplan_step_kernel(int NA, int i, int loop, const double *Pobs, int n_obs,
                                                  const double *pos_cur, double *pos_next, double *st, double *Pr,
                                                  double *Prd);

// ---- srb_sim.hip
extern "C" __global__ void srb_sim_advance_kernel(int n_agents, int N, int C, int nv, double Ts, double vref, int c,
                                                  int c_first, double *state, const double *goal, const int *phase,
                                                  const double *x, const int *status, const int *iters, double *x0,
                                                  double *ref, double *foot, double *last_state, double *alpha_buf,
                                                  double *plan_table, double *traj, int *status_log, int *iters_log,
                                                  double *x_log);
// srb_plant.hip (compiled as part of srb_sim.hip): the advance of a cycle c > c_first through the disturbed plant of
// srb_plant -- srb_sim_advance_kernel's arguments, then the row offset of the tables, gravity, the seed's halves
// and the struct's tables (each may be null, n_push 0)
extern "C" __global__ void srb_sim_advance_plant_kernel(
    int n_agents, int N, int C, int nv, double Ts, double vref, int c, int c_first, double *state, const double *goal,
    const int *phase, const double *x, const int *status, const int *iters, double *x0, double *ref, double *foot,
    double *last_state, double *alpha_buf, double *plan_table, double *traj, int *status_log, int *iters_log,
    double *x_log, int agent_offset, double grav, unsigned seed_lo, unsigned seed_hi, const double *kick_v,
    const double *kick_p, const double *plant_hcom, int n_push, const int *push_cycle, const int *push_agent,
    const double *push_dv, double *dist_log);
// srb_link.hip: the degraded neighbour link (srb_link), one cycle's update of all n_all rows.  slot_c: the ring slot
// of cycle c, (c - c_first) mod (max_delay + 1); age_row: age_log's row of cycle c or null.  LPR threads per row:
// launch it through srb_launch_link_update (the grid follows from lanes)
#define SRB_LINK_LANES 8                 // srb_link_update_device's mapping (measured: DESIGN.md 10.14)
int srb_launch_link_update(int lanes, int n_all, int N, double Ts, int c, int c_first, int max_delay, int slot_c,
                           int extrapolate, unsigned seed_lo, unsigned seed_hi, const int *delay, const double *drop,
                           const double *noise_p, const double *noise_v, const double *last_state,
                           const double *plan_table, double *ring_state, double *ring_plan, double *held_state,
                           double *held_plan, int *held_cycle, double *seen_state, double *seen_plan, int *age_row,
                           hipStream_t s);
#define SRB_SIM_AGENTS_PER_BLOCK 16    // srb_sim_metrics_kernel: agents per block of 256 threads (16 threads each)
extern "C" __global__ void srb_sim_metrics_kernel(int n_agents, int c, int c_first, const double *state,
                                                  const double *obstacles, int n_obs, const double *nbr_state, int n_all,
                                                  int agent_offset, double *d_obs, double *d_agent, double *min_d_obs,
                                                  double *min_d_agent, int *fail_cycle, double *distance_to_fail);

// ---- srb_scenes.hip (srb_ctx_set_scenes): the selections over the sub-tables of the agent's scene, global indices
// out; the metrics with block b serving agents (b % blocks_per_scene) SRB_SIM_AGENTS_PER_BLOCK .. of scene
// scene0 + b / blocks_per_scene and staging only that scene's rows (obs_rows / nbr_rows a scene: scene_obs /
// scene_agents, or 0 without the table)
extern "C" __global__ void srb_knn_scene_kernel(int n_agents, const double *x0g, const double *obstacles,
                                                const double *nbr_state, int agent_offset, int scene_agents,
                                                int scene_obs, int K_obs, int K_nbr, int *sel_out, int sel_stride);
extern "C" __global__ void srb_knn_plan_scene_kernel(int n_agents, const double *x0g, const double *nbr_state,
                                                     const double *nbr_plan, int N, int agent_offset, int scene_agents,
                                                     int K_nbr, int *sel_out, int sel_stride, const double *own_plan);
extern "C" __global__ void srb_sim_scene_metrics_kernel(int n_agents, int c, int c_first, const double *state,
                                                        const double *obstacles, int obs_rows, const double *nbr_state,
                                                        int nbr_rows, int scene_agents, int agent_offset, int scene0,
                                                        int blocks_per_scene, double *d_obs, double *d_agent,
                                                        double *min_d_obs, double *min_d_agent, int *fail_cycle,
                                                        double *distance_to_fail);

// ---- srb_moving.hip (moving obstacles, srb_moving): the horizon-aware obstacle selection (whole table / the
// agent's scene, global indices out) and one control cycle of the obstacle table
extern "C" __global__ void srb_knn_obs_horizon_kernel(int n_agents, const double *x0g, const double *obstacles,
                                                      const double *obs_vel, int n_obs, int N, double Ts, int K_obs,
                                                      int *sel_out, int sel_stride);
extern "C" __global__ void srb_knn_obs_horizon_scene_kernel(int n_agents, const double *x0g, const double *obstacles,
                                                            const double *obs_vel, int N, double Ts, int agent_offset,
                                                            int scene_agents, int scene_obs, int K_obs, int *sel_out,
                                                            int sel_stride);
extern "C" __global__ void srb_obstacles_advance_kernel(int n_obs, double Ts, double *obstacles, const double *obs_vel);

// ---- srb_sizes.hip (obstacle sizes, srb_sizes): the clearance selection (whole table / the agent's scene, global
// indices out; obs_vel null: the distance now) and the metrics with a body radius per obstacle row
extern "C" __global__ void srb_knn_obs_clear_kernel(int n_agents, const double *x0g, const double *obstacles,
                                                    const double *obs_vel, const double *obs_eps, int n_obs, int N,
                                                    double Ts, int K_obs, int *sel_out, int sel_stride);
extern "C" __global__ void srb_knn_obs_clear_scene_kernel(int n_agents, const double *x0g, const double *obstacles,
                                                          const double *obs_vel, const double *obs_eps, int N, double Ts,
                                                          int agent_offset, int scene_agents, int scene_obs, int K_obs,
                                                          int *sel_out, int sel_stride);
extern "C" __global__ void srb_sim_metrics_sized_kernel(int n_agents, int c, int c_first, const double *state,
                                                        const double *obstacles, const double *obs_radius, int n_obs,
                                                        const double *nbr_state, int n_all, int agent_offset,
                                                        double *d_obs, double *d_agent, double *min_d_obs,
                                                        double *min_d_agent, int *fail_cycle, double *distance_to_fail);
extern "C" __global__ void srb_sim_scene_metrics_sized_kernel(int n_agents, int c, int c_first, const double *state,
                                                              const double *obstacles, const double *obs_radius,
                                                              int obs_rows, const double *nbr_state, int nbr_rows,
                                                              int scene_agents, int agent_offset, int scene0,
                                                              int blocks_per_scene, double *d_obs, double *d_agent,
                                                              double *min_d_obs, double *min_d_agent, int *fail_cycle,
                                                              double *distance_to_fail);

// ---- srb_agents.hip (agent sizes, srb_agent_sizes): the neighbour columns by clearance dist_i - agent_rad[i] (whole
// table / the agent's scene, global indices out; nbr_plan null: the snapshot distance, else knn_plan_select's
// minimum over the horizon) and the metrics with a body radius per agent row (obs_radius may be null: srb_sim's
// obstacle half; collide_cycle may be null)
extern "C" __global__ void srb_knn_nbr_clear_kernel(int n_agents, const double *x0g, const double *nbr_state,
                                                    const double *nbr_plan, const double *agent_rad, int n_all, int N,
                                                    int agent_offset, int K_nbr, int *sel_out, int sel_stride);
extern "C" __global__ void srb_knn_nbr_clear_scene_kernel(int n_agents, const double *x0g, const double *nbr_state,
                                                          const double *nbr_plan, const double *agent_rad, int N,
                                                          int agent_offset, int scene_agents, int K_nbr, int *sel_out,
                                                          int sel_stride);
extern "C" __global__ void srb_sim_metrics_agents_kernel(int n_agents, int c, int c_first, const double *state,
                                                         const double *obstacles, const double *obs_radius, int n_obs,
                                                         const double *nbr_state, const double *agent_body, int n_all,
                                                         int agent_offset, double *d_obs, double *d_agent,
                                                         double *min_d_obs, double *min_d_agent, int *fail_cycle,
                                                         double *distance_to_fail, int *collide_cycle);
extern "C" __global__ void srb_sim_scene_metrics_agents_kernel(int n_agents, int c, int c_first, const double *state,
                                                               const double *obstacles, const double *obs_radius,
                                                               int obs_rows, const double *nbr_state,
                                                               const double *agent_body, int nbr_rows, int scene_agents,
                                                               int agent_offset, int scene0, int blocks_per_scene,
                                                               double *d_obs, double *d_agent, double *min_d_obs,
                                                               double *min_d_agent, int *fail_cycle,
                                                               double *distance_to_fail, int *collide_cycle);

// ---- srb_llctrl.hip
extern "C" __global__ void srb_ll_kernel(SrbLLKParams prm, int n_agents, SrbLLDev io);

// ---- srb12_kernels.hip
#define SRB_DECL12(TL, TO, NC, K1)                                                                             \
    extern "C" __global__ void srb12_kernel_##TL##_##TO##_##NC##_##K1(                                       \
        Srb12KParams prm, int n_agents, const double *x0g, const double *xrefg, const double *footg,           \
        const int *contactg, const double *obstacles, const double *nbr_state, const int *sel_g,              \
        double *x_qp_out, double *x_out, double *obj_out, int *status_out, int *iters_out,                    \
        const double *nbr_plan, double *plan_out);
SRB12_INSTANCES(SRB_DECL12)
#undef SRB_DECL12
// the table instances (srb12_kernels.hip under -DSRB12_MOVING): five more arguments, the velocity table of srb_moving,
// the level table of srb_sizes, the safety-radius and pad tables of srb_agent_sizes (each may be null) and the
// agent_offset of the agent tables' own row
#define SRB_DECL12_MV(TL, TO, NC, K1)                                                                          \
    extern "C" __global__ void srb12_kernel_mv_##TL##_##TO##_##NC##_##K1(                                    \
        Srb12KParams prm, int n_agents, const double *x0g, const double *xrefg, const double *footg,           \
        const int *contactg, const double *obstacles, const double *nbr_state, const int *sel_g,              \
        double *x_qp_out, double *x_out, double *obj_out, int *status_out, int *iters_out,                    \
        const double *nbr_plan, double *plan_out, const double *obs_vel, const double *obs_eps,               \
        const double *agent_rad, const double *agent_pad, int agent_offset);
SRB12_INSTANCES(SRB_DECL12_MV)
#undef SRB_DECL12_MV
extern "C" __global__ void srb12_pos_kernel(int n_agents, const double *x0g, double *pos);

// ---- srb12_sim.hip: one thread per (agent, grid), n_agents N threads
extern "C" __global__ void srb12_sim_advance_kernel(int n_agents, int N, double Ts, double vref, double hcom,
                                                    double yaw_step, double hold_radius, int gait, int c, int c_first,
                                                    double *state, const double *goal, const int *phase,
                                                    const double *x, const int *status, const int *iters, double *x0,
                                                    double *xref, double *foot, int *contact, double *last_state,
                                                    double *com, double *traj, int *status_log, int *iters_log,
                                                    double *x_log);
// ---- srb12_plant.hip (compiled inside srb12_sim.hip): the disturbed plant, cycles c > c_first.  The state kernel is one
// thread per agent, the advance one per (agent, grid) as srb12_sim_advance_kernel, whose arguments it takes
struct Srb12PlantIb { double v[9]; };                     // the model's body inertia, row-major, by value
extern "C" __global__ void srb12_plant_state_kernel(int n_agents, int N, double Ts, double mass, Srb12PlantIb Ib,
                                                    double grav, int c, int c_first, double *state, const double *x,
                                                    const double *xref, const double *foot, const int *contact,
                                                    int agent_offset, unsigned seed_lo, unsigned seed_hi,
                                                    const double *kick_v, const double *kick_p, const double *kick_w,
                                                    const double *plant_mass, const double *plant_inertia, int at_state,
                                                    int roll, int n_push, const int *push_cycle, const int *push_agent,
                                                    const double *push_dv, double *dist_log);
extern "C" __global__ void srb12_sim_advance_plant_kernel(int n_agents, int N, double Ts, double vref, double hcom,
                                                          double yaw_step, double hold_radius, int gait, int c,
                                                          int c_first, double *state, const double *goal,
                                                          const int *phase, const double *x, const int *status,
                                                          const int *iters, double *x0, double *xref, double *foot,
                                                          int *contact, double *last_state, double *com, double *traj,
                                                          int *status_log, int *iters_log, double *x_log);
// last cycle's plans as this cycle's table (dist.shift_plans), one thread per (agent, grid)
extern "C" __global__ void srb12_plan_shift_kernel(int n_agents, int N, int grids, const double *plan, double *table);
