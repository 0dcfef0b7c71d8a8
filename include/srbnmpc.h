/*
 * srbnmpc -- batched CBF-NMPC solver for AMD Instinct MI355X (gfx950).  C ABI.
 *
 * Drop-in replacement for the per-control-cycle solve of the HDSRL/SRB-CBF-NMPC
 * reference (MPC_dist::run_NMPC, /root/reference/src/MPC_dist.cpp:81-454):
 *   - the QP stage iswiftQp_e(Q_qp, f_qp, Aeq, beq, Gineq, hineq, sol)
 *       (/root/reference/optimization/iSWIFT/cpp_wrapper/iswift_qp.h:14-16, called at
 *        MPC_dist.cpp:348), and
 *   - the NLP stage nlp.AddVariableSet/AddConstraintSet/AddCostSet + SnoptSolver::Solve
 *       (MPC_dist.cpp:402-427 with include/dec_vars_constr_cost.h),
 * for a whole batch of agents per call.  Problem assembly (MPC_dist.cpp:99-321) and the
 * closest-obstacle scan (:371-396) happen on the device from the per-agent inputs below.
 *
 * Conventions: plain C, fp64, agent-major arrays, caller-owned buffers, int status
 * codes (0 = success; negative = API error), no exceptions across the ABI.  Solver exit
 * codes mirror iSWIFT's (GlobalOptions.h:31-34): 0 OPTIMAL, 1 KKTFAIL, 2 MAXIT, 3 FATAL.
 * As in the reference (iswift_qp.cpp:126-151, MPC_dist.cpp:421), a non-optimal exit
 * still returns the last iterate.
 *
 * Decision vector of one agent (the reference's mpc_state_eventbased_, MPC_dist.cpp:345):
 *   x = [ X (4N: x, xdot, y, ydot per grid) | U (2N: CoP) | lambda (C*N) | s ]
 *   nv = (6 + C) * N + 1
 */
#ifndef SRBNMPC_H
#define SRBNMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define SRB_OK 0
#define SRB_ERR_ARG (-1)
#define SRB_ERR_HIP (-2)
#define SRB_ERR_SIZE (-3)

/*
 * ABI versioning.  Every I/O struct (srb_batch, srb_prep, srb_sim, srb_ll_io) starts with
 * `int struct_size`, which the caller sets to sizeof(struct) of the header it was compiled
 * against; the library rejects any other value with SRB_ERR_ARG (srb_last_error() names
 * the struct), so a caller built against an older or newer layout fails loudly instead of
 * having trailing fields read from whatever follows its struct.  srb_abi_version() returns
 * the SRB_ABI_VERSION the library was built with (bumped on any layout change).
 *   srb_batch b = {sizeof(srb_batch)};      (C)      srb_batch b{}; b.struct_size = sizeof b;  (C++)
 */
#define SRB_ABI_VERSION 6
int srb_abi_version(void);

/* solver exit codes (iSWIFT GlobalOptions.h:31-34) */
#define SRB_OPTIMAL 0
#define SRB_KKTFAIL 1
#define SRB_MAXIT 2
#define SRB_FATAL 3

typedef struct srb_params {
    int N;              /* grid points in the horizon (reference: 4, MPC_dist.cpp:92)               */
    int C;              /* stance contacts per grid (trot 2, stand 4; MPC_dist.cpp:132)             */
    int K_obs;          /* nearest static obstacles per agent (reference: 1, MPC_dist.cpp:371-396)  */
    int K_nbr;          /* nearest other agents used as moving obstacles (reference: 0)             */
    double grav, hcom, Ts, mu;       /* 9.81, 0.29, 0.043, 0.7 (MPC_dist.cpp:90-104)                */
    double Qw, Pw, Rw, Sw;           /* 300, 2000, 0.1, 3000 (MPC_dist.cpp:172-175)                 */
    double box;                      /* 1e3 (MPC_dist.cpp:317-318)                                  */
    double eps_obs, eps_nbr;         /* (double)1.9f, (double)2.2f (dec_vars_constr_cost.h:401-402) */
    double vsat;                     /* (double)0.35f (dec_vars_constr_cost.h:306-307)              */
    double tol;                      /* 1e-6 (GlobalOptions.h:24-25)                                */
    int qp_maxit, nlp_maxit;         /* 25 (GlobalOptions.h:23), 50                                 */
    int use_nlp;                     /* MPC_dist::use_snopt (MPC_dist.hpp:139): 0 = QP only         */
} srb_params;

/* Reference defaults for horizon N and C contacts (K_obs = 1, K_nbr = 0, use_nlp = 1). */
void srb_params_default(srb_params *p, int N, int C);
int srb_nv(const srb_params *p);     /* (6+C)N+1 */

/*
 * One batch.  All pointers agent-major, fp64 unless noted.
 *   x0        [A][4]        x, xdot, y, ydot             (MPC_dist.cpp:226-229; q[0],dq[0],q[1],dq[1])
 *   ref       [A][4N]       com_desired_Traj_vec         (copPlanner_eventbase, MPC_dist.cpp:780)
 *   foot      [A][N][2][C]  stance footholds per grid: row 0 = x, row 1 = y of the C
 *                           contact legs in FR,FL,RR,RL order (footholdsPlanner, :1238-1260)
 *   obstacles [n_obs][2]    Pobs_real columns, shared by the batch (MPC_dist.hpp:85)
 *   nbr_state [n_all][4]    get_lastState() of every agent: x, y, xdot, ydot (MPC_dist.cpp:1272-1276);
 *                           may be NULL when K_nbr == 0.  Local agent a is global agent
 *                           agent_offset + a (itself excluded from its neighbours).
 * Outputs:
 *   x_qp      [A][nv]       QP-stage solution (qp_solution_eventbased_, :350-354); may be NULL.  With the NLP
 *                           stage on it is the NLP's warm start, solved to SRB_OPT_QP_WARM_TOL (default 0.3,
 *                           status 4 below), not to iSWIFT's 1e-6 -- set that option to 0 for the reference's
 *                           point (the MPC_dist shims do); srb_solve_qp always solves to 1e-6
 *   x         [A][nv]       final decision vector (mpc_state_eventbased_ after :423-426)
 *   obj       [A]           0.5 x'Q_qp x + f'x (ExCost::GetCost)
 *   status    [A][2] int    QP, NLP exit codes: 0 OPTIMAL, 1 KKTFAIL, 2 MAXIT, 3 FATAL (iSWIFT's);
 *                           QP also 4 QP_WARM: converged at the warm-start tolerance only (the NLP follows);
 *                           NLP also 4 ACCEPTABLE: stopped at a near-optimal iterate (primal and
 *                           complementarity met, dual residual within 100x of its threshold)
 *                           whose next step was blocked or needed an inertia shift, or met only
 *                           the loosened exit tests the polish relies on and was not polished
 *                           (rejected, or SRB_OPT_POLISH = 0); 3 FATAL also when a dual passes 1e10
 *                           (infeasible rows) -- the iterate returned is finite in every case
 *   iters     [A][2] int    QP, NLP interior-point iterations
 * Bezier fit of the predicted CoM (fitComTrajectory_eventbase, MPC_dist.cpp:784-855), fused
 * into the solve; both NULL = not fitted (needs N >= 4):
 *   alpha_buf [A][4]        mpc_state_alpha_buffer_ (the previous solve's X_3; the start
 *                           position with zero velocity before the first one, :792, :798)
 *   alpha     [A][20]       get_alphaCOM(): 4 x 5 row-major (state row, Bernstein index)
 * Selected obstacle rows (the closest-obstacle scan, MPC_dist.cpp:371-382), optional:
 *   sel       [A][Ko + Kn] int  out: the Ko = min(K_obs, n_obs) static obstacle indices, then the
 *                           Kn = min(K_nbr, n_all - 1) neighbour rows (global indices into
 *                           nbr_state; -1 = none), in the reference's scan order (sqrt distance,
 *                           lower index on ties; a static round with nothing closer than 1000 m
 *                           selects obstacle 0, as min_dist = 1000 / min_i = 0 do).  NULL = the
 *                           context's own scratch buffer.
 * Neighbour plans (the inter-agent CBF rows against what the neighbours plan to do), both optional:
 *   nbr_plan  [n_all][N][2] in: row i, grid k is global agent i's predicted (x, y) at time (k+1) Ts from the
 *                           instant of x0 -- the grid times of obstacle row k.  NULL: the neighbour rows are
 *                           the constant-velocity guess p + v Ts (k+1) from nbr_state.  Read only by the NLP
 *                           stage and only for the neighbour columns of sel; needs nbr_state (the selection's
 *                           snapshot) and, with K_nbr > 0, agent_offset + n_agents <= n_all.  Row
 *                           agent_offset + a is agent a's own previous plan: the horizon-aware selection
 *                           (SRB_OPT_PLAN_SELECTION) reads it, the CBF rows never do.
 *   plan      [A][N][2]     out: (x[4k], x[4k+2]) of the returned x for every agent, whatever its status (written
 *                           by the kernel that writes the final x: always a gather of x).  srb_solve_qp
 *                           writes it from the QP x.  Must not overlap the nbr_plan table: workgroups read the
 *                           table while others write their plans, so an iteration over plans needs two buffers.
 */
typedef struct srb_batch {
    int struct_size;         /* sizeof(srb_batch) (ABI check, see SRB_ABI_VERSION) */
    const double *x0, *ref, *foot, *obstacles, *nbr_state;
    int n_obs, n_all, agent_offset;
    double *x_qp, *x, *obj;
    int *status, *iters;
    const double *alpha_buf;
    double *alpha;
    int *sel;
    int obstacles_version;   /* != 0: the obstacle table is unchanged since the last call that passed
                                this version, pointer and n_obs (the reference's Pobs_real is set once,
                                MPC_dist::setPobs_real): its selection grid is reused; 0: rebuilt */
    const double *nbr_plan;  /* [n_all][N][2] neighbour plans, or NULL (constant velocity) */
    double *plan;            /* [A][N][2] this batch's plans, or NULL */
} srb_batch;

typedef struct srb_ctx srb_ctx;

/* Create a context on HIP device `device` for batches of up to max_agents agents. */
int srb_ctx_create(const srb_params *p, int max_agents, int device, srb_ctx **out);
int srb_ctx_destroy(srb_ctx *ctx);

/* Waves (64-lane wavefronts) per agent's workgroup: 0 = automatic (4 while the batch has no
 * more agents than the device has CUs, else 1, or 2 for problems whose row slots exceed five
 * per lane), or force 1, 2 or 4.  Results are bit-identical for a given wave count; different
 * counts sum the reduced Newton matrix in a different order (round-off differences only).
 * srb_ctx_waves() returns the count the last launch used. */
int srb_ctx_set_waves(srb_ctx *ctx, int nw);
int srb_ctx_waves(srb_ctx *ctx);

/* The kernels the last launch of srb_solve_batch* / srb_solve_qp* ran, by name (read only; the strings are static
 * storage): *solve the solve kernel (srb_nmpc_kernel_<NZL>_<TS>_<NW>_<NC>_<CC>_<KC>, its _mv_ form when a table of
 * srb_moving / srb_sizes / srb_agent_sizes was given, its f32_ form under SRB_OPT_KKT_FP32_MU), *polish the polish
 * kernel launched after it (srb_polish_kernel[_mv]_*), or "" where the polish ran fused into the solve kernel or
 * not at all.  The record is written where the kernels are launched, not recomputed; "" before the first launch.
 * The polish kernel is the solve instance's own only when SRB_OPT_POLISH_WAVES equals the solve's waves: at the
 * default (0) a one-wave solve is polished by the two-wave instance of the same NZL.  Either pointer may be NULL. */
int srb_ctx_last_kernels(srb_ctx *ctx, const char **solve, const char **polish);
/* The shipped solve-kernel instances, host only (no device needed): entry i's dims (NZL, TS, NW, NC, CC, KC: the
 * reduced-system bound, slot trips per thread, waves per agent and the compiled shape N, C, K_obs + K_nbr, 0 = read
 * at run time) and its solve kernel's name; the fp32-factor entries follow the fp64 ones.  SRB_ERR_ARG past the end. */
int srb_kernel_table(int i, int dims[6], const char **name);
/* The dims of the fp64 instance a launch of problem p wanting `waves` (1, 2 or 4) waves per agent picks, with
 * 160 KiB of LDS per workgroup; host only.  SRB_ERR_SIZE where no instance fits. */
int srb_pick_kernel(const srb_params *p, int waves, int dims[6]);
/* The parameter checks of srb_ctx_create alone, host only: SRB_OK, or the error srb_ctx_create would return
 * (srb_last_error() says why). */
int srb_check_params(const srb_params *p);

/* Scenes: the batch is a set of independent teams of scene_agents agents, each with scene_obs obstacle rows.
 * Global agent g = agent_offset + a belongs to scene g / scene_agents.  Its static rows are selected from
 * obstacles[scene*scene_obs .. +scene_obs), its neighbour rows from nbr_state (and nbr_plan) rows
 * [scene*scene_agents .. +scene_agents), itself excluded.  sel holds GLOBAL row indices (-1 as before).
 * (0, 0) = off (default): one team, today's behaviour bit for bit.
 * Tables stay flat and scene-major; n_obs and n_all stay the total row counts.  Honoured by srb_solve_batch,
 * srb_solve_qp, srb_solve_batch_device, srb_select_device (tables 1, 2, 3 and the horizon-aware selection),
 * srb_sim_metrics_device (nearest obstacle / other agent of the agent's scene) and srb_rollout_device.
 * K_obs clamps to scene_obs and K_nbr to scene_agents - 1 (batch-uniform, like the n_obs / n_all - 1 clamps);
 * the static 1000 m rule selects the scene's row 0 (global scene*scene_obs).  Scene tables are scanned brute
 * force: no selection grid is built or consulted, and a cached static grid stays as it is.
 * A call is refused (SRB_ERR_ARG, before anything is launched) when n_all is not a multiple of scene_agents,
 * when n_obs != scenes * scene_obs with both tables in use, when agent_offset + n_agents lies beyond the last
 * scene, and, for srb_rollout_device, when n_agents is not a multiple of scene_agents.  A shard (agent_offset,
 * n_all > n_agents) may start and end inside a scene.  set refuses a negative value and scene_agents == 0 with
 * scene_obs != 0.  The SRB-12 mode has the same partition on its own context (srb12_ctx_set_scenes); the
 * MPC_dist shims have no scenes. */
int srb_ctx_set_scenes(srb_ctx *ctx, int scene_agents, int scene_obs);
int srb_ctx_scenes(srb_ctx *ctx, int *scene_agents, int *scene_obs);

/* Context options (no environment variable changes what the library computes; every knob is one
 * of these, per context).  set returns SRB_ERR_ARG for an unknown option or a value out of range.
 *   SRB_OPT_POLISH               1 (default) polish the NLP result to the exact KKT point of its active
 *                                set, 0 off: results that met only the loosened NLP exit
 *                                tests then stay ACCEPTABLE (4)
 *   SRB_OPT_POLISH_RHO           the polish's regularisation 1 / rho (default 1e9; 1e3 .. 1e12)
 *   SRB_OPT_POLISH_WAVES         waves per agent of the polish kernel: 0 automatic (default), 1, 2, 4
 *   SRB_OPT_GRID_MIN_ROWS        tables of this many rows or more get a selection grid (default 8192)
 *   SRB_OPT_GRID_MIN_ROWS_STATIC the same for a versioned static obstacle table (default 4096)
 *   SRB_OPT_POLISH_FUSED         1 (default) the polish runs at the end of the solve kernel (problems with
 *                                N(C-1)+1 <= 16), 0 as a kernel of its own after it; the same results
 *   SRB_OPT_LAST_POLISH          read only: how the last launch polished, 0 not at all, 1 polish kernel,
 *                                2 fused into the solve kernel
 *   SRB_OPT_TIMING               1 (default): HIP events around the launch's kernels (srb_last_kernel_ms,
 *                                srb_last_polish_ms); 0: none (each event record is a marker the queue
 *                                drains to: a few us per call, measured in bench.py's timed loop)
 *   SRB_OPT_QP_WARM_TOL          the QP stage's tolerance when the NLP stage follows (default 0.3; 0: the
 *                                full tolerance, 1e-6 as iSWIFT): that point only warm-starts the NLP, whose
 *                                result is unchanged (the polish makes it exact; statuses and NLP iterations
 *                                unchanged on the bench batches) while the QP stage takes 3.0 instead of 5.8
 *                                iterations at configs[2]; x_qp is then that rougher point.  The
 *                                QP-only solve (srb_solve_qp, use_nlp = 0) always runs to the full tolerance.
 *                                Such a QP stage reports status 4 (QP_WARM: converged at this tolerance), never
 *                                0; with 0 here it reports iSWIFT's codes (0 OPTIMAL at 1e-6)
 *   SRB_OPT_SELECTION            1 (default): srb_solve_batch_device runs the obstacle / neighbour selection
 *                                itself; 0: the caller has filled batch.sel with srb_select_device (the two
 *                                tables may then be selected on either side of the neighbour all-gather)
 *   SRB_OPT_KKT_FP32_MU          0 (default): the reduced Newton matrix is inverted in fp64.  > 0: BASELINE
 *                                configs[4]'s "fp32 KKT with fp64 iterative-refine residuals" -- where the
 *                                instance has an fp32-factor variant (the configs[2] and config-5 shapes), the
 *                                matrix (assembled in fp64) is inverted in fp32 while the complementarity mu is
 *                                above this value, each solve then refined SRB_OPT_KKT_FP32_REFINE times (default
 *                                3) against the fp64 matrix; fp64 below it
 *   SRB_OPT_LAST_KKT_FP32        read only: 1 if the last launch ran an fp32-factor instance
 *   SRB_OPT_PLAN_SELECTION       0 (default): neighbours are selected from the snapshot (nbr_state), nearest now.
 *                                1: by closest predicted approach over the horizon (srb_knn_plan_kernel): the key
 *                                of table row i for agent g = agent_offset + a is the square root of the smallest
 *                                squared distance over the snapshot pair (x0 against nbr_state[i]) and the N grid
 *                                pairs nbr_plan[g][k] against nbr_plan[i][k]; same order, ties, NaN and -1 rules,
 *                                brute force.  Needs batch.nbr_plan (SRB_ERR_ARG without it); the static columns
 *                                are selected as before */
#define SRB_OPT_POLISH 1
#define SRB_OPT_POLISH_RHO 2
#define SRB_OPT_POLISH_WAVES 3
#define SRB_OPT_GRID_MIN_ROWS 4
#define SRB_OPT_GRID_MIN_ROWS_STATIC 5
#define SRB_OPT_POLISH_FUSED 6
#define SRB_OPT_LAST_POLISH 7
#define SRB_OPT_TIMING 8
#define SRB_OPT_QP_WARM_TOL 9
#define SRB_OPT_SELECTION 10
#define SRB_OPT_KKT_FP32_MU 11
#define SRB_OPT_KKT_FP32_REFINE 12
#define SRB_OPT_LAST_KKT_FP32 13
#define SRB_OPT_PLAN_SELECTION 14
int srb_ctx_set_option(srb_ctx *ctx, int opt, double value);
int srb_ctx_get_option(srb_ctx *ctx, int opt, double *value);

/* QP-stage starting point: 1 (default) the scaled start s = max(h - Gx, 0.1), z = 1/s from the
 * least-squares x of iSWIFT's kkt_initialize (Auxilary.c:680-755); 0 iSWIFT's own shifted start
 * (z + 1 + max(h - Gx): ~1e3 with the +-1e3 boxes of MPC_dist.cpp:317-318), which follows the
 * genuine iSWIFT step for step (tests/test_gpu_parity.py) but needs up to twice the iterations on
 * the slowest agents.  Both end at the QP optimum to the solver tolerance. */
int srb_ctx_set_qp_init(srb_ctx *ctx, int mode);

/* Host buffers: copies in, solves, copies out, synchronises.  n_agents <= max_agents. */
int srb_solve_batch(srb_ctx *ctx, int n_agents, const srb_batch *host_io);

/* Same as srb_solve_batch with use_nlp forced to 0 (reference use_snopt == false). */
int srb_solve_qp(srb_ctx *ctx, int n_agents, const srb_batch *host_io);

/* Device buffers (all pointers in `dev_io` are device pointers), asynchronous on
 * `stream` (a hipStream_t; NULL = the HIP null stream, which orders against every blocking
 * stream, as the CUDA/HIP convention has it).  Pass the stream that produced the inputs (the
 * Python layer passes torch's current stream, whose default is that null stream).  Call
 * srb_sync() or synchronise the stream.
 *
 * Ordering.  A context executes its calls in submission order, whatever stream each call
 * names: a launch on a stream other than the previous call's first waits (hipStreamWaitEvent)
 * for that call's work, and the host entry points (srb_solve_batch / srb_solve_qp) order
 * after the last device launch the same way.  The context's scratch -- the selection grids
 * and their static-table cache, the default `sel` buffer, the staging buffers and the timing
 * events -- is therefore never used by two launches in flight.  For solves that run
 * concurrently, use one context per stream. */
int srb_solve_batch_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, void *stream);

/* The selection alone (MPC_dist.cpp:371-396 generalised to K), asynchronous on `stream`: tables = 1 the static
 * obstacles (columns 0 .. Ko-1 of dev_io->sel), 2 the neighbour snapshot (columns Ko .. Ko+Kn-1), 3 both.
 * With SRB_OPT_PLAN_SELECTION = 1, tables & 2 is the horizon-aware selection and needs dev_io->nbr_plan.
 * dev_io->sel is required; the other members are read as srb_solve_batch_device reads them.  Multi-GPU use
 * (bench.py): select the static obstacles while the neighbour all-gather is in flight, the neighbours after
 * it, then solve with SRB_OPT_SELECTION = 0.  Indices are identical to the solve's own selection. */
int srb_select_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, int tables, void *stream);
int srb_sync(srb_ctx *ctx);

/*
 * Input assembly on the device (the planners run_NMPC calls before its solve; SURVEY.md 8(f)
 * row 2), one batch of agents, asynchronous on `stream` like srb_solve_batch_device:
 *   updateState + x0 (MPC_dist.cpp:1195-1202, :226-229), get_lastState (:1272-1276),
 *   copPlanner_eventbase (:702-782) and footholdsPlanner (:1204-1266).
 * All pointers are device pointers.  Inputs:
 *   Pr, Prd      [T][n_rows]   the HL path Pr_refined_ / Prd_refined_ (2*NA x T, column-major as
 *                              Eigen stores it); agent id uses rows 2 id, 2 id + 1
 *   agent_id     [A] int       (NULL: agent_offset + a)
 *   gait_domain  [A] int       gaitDomain_: the window starts at column 4 * gaitDomain_ (NDOMAIN
 *                              grids per domain) and spans N columns
 *   contact      [A][4] int    contactInd (FR, FL, RR, RL); must give C contacts
 *   toe          [A][3][4]     toePos (row-major 3 x 4)
 *   start        [A][2]        agent_Initial_ (default stance while gaitDomain_ <= 1)
 *   q, dq        [A][18]       generalised coordinates / velocities (q[0], q[1], dq[0], dq[1] used)
 * Outputs: x0 [A][4], ref [A][4N], foot [A][N][2][C] (the srb_batch inputs), last_state [A][4]
 * (the neighbour-snapshot row), status [A] int: 0 ok, 1 contact pattern does not give C
 * contacts, 2 reference window outside the path.
 */
typedef struct srb_prep {
    int struct_size;         /* sizeof(srb_prep) (ABI check) */
    const double *Pr, *Prd;
    int n_rows, T, agent_offset;
    const int *agent_id, *gait_domain, *contact;
    const double *toe, *start, *q, *dq;
    double *x0, *ref, *foot, *last_state;
    int *status;
} srb_prep;
int srb_prepare_batch_device(srb_ctx *ctx, int n_agents, const srb_prep *dev_io, void *stream);

/*
 * Closed-loop team rollout on the device: the step from one cycle's solution to the next cycle's inputs, and the
 * team's safety log, so that T control cycles run without a host round trip.  One cycle is
 * one gait domain of NDOMAIN = 4 grids (global_loco_opts.h:9), so N >= 4.  The plant of these entry points is nominal
 * (srb_plant, further down, disturbs it through entry points of its own): the state that
 * starts cycle c + 1 is the X the solve of cycle c predicted at grid index 3, the domain's end -- what the
 * reference buffers (MPC_dist.cpp:798) -- whatever that solve's status.  All pointers are device pointers, fp64
 * unless noted; cycles count from c_first, and log rows are indexed by c - c_first.
 *
 * srb_sim_advance_device(ctx, A, sim, c, stream), cycle c >= c_first:
 *   state       [A][4]       x, xdot, y, ydot.  c == c_first: read (the caller's start state); later cycles:
 *                            written from x[a][12..15]
 *   goal        [A][2]       in: each agent's goal
 *   phase       [A] int      in, optional: added to c for the trot parity
 *   vref                     reference speed (the synthetic workload's: 0.27)
 *   x, status, iters         in: the previous solve's outputs (srb_batch layout); x is required when c != c_first
 *   x0 [A][4], ref [A][4N], foot [A][N][2][C]  out: the srb_batch inputs of cycle c.  ref is the straight line
 *                            from the current position to the goal at v = min(vref, dist / (Ts N)), so it never
 *                            overshoots and an agent at its goal gets a standing reference; foot is the default
 *                            stance (MPC_dist.cpp:1206-1209) around the reference position at each domain's
 *                            start, legs {FR,RL} when c + phase + k / 4 is even, {FL,RR} when odd (C = 2), all
 *                            four for C = 4
 *   last_state  [A][4]       out: x, y, xdot, ydot -- the neighbour-snapshot row (get_lastState)
 *   alpha_buf   [A][4]       out, optional: the state, as the Bezier buffer of the solve
 *   plan_table  [A][N][2]    out, optional, c != c_first only: the previous solve's plans (x[4k], x[4k+2]) shifted
 *                            by 4 grids; past the horizon the last finite difference continues,
 *                            last + m (last - previous).  At c_first the caller's content stands
 *   traj        [T+1][A][4]  out, optional: row c - c_first gets the state
 *   status_log, iters_log [T][A][2] int, x_log [T][A][nv]  out, optional, c != c_first only: row c - c_first - 1
 *                            gets the previous solve's status, iters, x
 * srb_sim_metrics_device(ctx, A, sim, c, stream): the safety metrics of `state` at the start of cycle c, brute
 * force and independent of the solver's own selection:
 *   obstacles [n_obs][2], nbr_state [n_all][4], agent_offset   in: as in srb_batch (row agent_offset + a is the
 *                            agent itself and is left out); either table may be empty
 *   d_obs, d_agent [A]       out, optional: distance to the nearest obstacle / other agent at this cycle; a table
 *                            row holding a NaN never wins, an empty table gives +inf
 *   min_d_obs, min_d_agent [A]  out, optional: their minima over the cycles c_first .. c
 *   fail_cycle [A] int, distance_to_fail [A]  out, optional: the first cycle with d_obs < 0.5 (else -1) and
 *                            sqrt(x^2 + y^2) at that cycle (else 0): updateDistance_to_fail, MPC_dist.cpp:21-40;
 *                            once set they are never overwritten.  The running results are initialised by the
 *                            call with c == c_first
 * Both are asynchronous on `stream` and ordered by the context like srb_solve_batch_device.
 *
 * srb_rollout_device(ctx, A, batch, sim, cycles, stream): `cycles` whole cycles of one team on one GPU.  For
 * c = c_first .. c_first + cycles - 1 it enqueues advance, metrics and solve, then one final advance that
 * flushes the last logs and the end state -- plain launches, no graph capture, no host synchronisation.  The two
 * structs are wired together here: the solve reads sim's x0, ref, foot, alpha_buf (when batch.alpha is set) and
 * sim.last_state as its nbr_state with n_all = A, agent_offset = 0; the advance reads batch's x, status, iters;
 * the metrics read batch's obstacles / n_obs and sim.last_state.  The members of either struct that this
 * replaces are ignored; batch.n_all / agent_offset must be A / 0 or both 0 (a shard cannot roll out alone: its
 * neighbours move too).  The first solve reads batch.nbr_plan (or none); with sim.plan_table set every later
 * solve reads that table as nbr_plan, so it must not overlap batch.plan.
 */
typedef struct srb_sim {
    int struct_size;         /* sizeof(srb_sim) (ABI check) */
    double *state;
    const double *goal;
    const int *phase;
    double vref;
    int c_first;
    const double *x;
    const int *status, *iters;
    double *x0, *ref, *foot, *last_state, *alpha_buf, *plan_table;
    double *traj;
    int *status_log, *iters_log;
    double *x_log;
    const double *obstacles, *nbr_state;
    int n_obs, n_all, agent_offset;
    double *d_obs, *d_agent, *min_d_obs, *min_d_agent;
    int *fail_cycle;
    double *distance_to_fail;
} srb_sim;
int srb_sim_advance_device(srb_ctx *ctx, int n_agents, const srb_sim *dev_io, int cycle, void *stream);
int srb_sim_metrics_device(srb_ctx *ctx, int n_agents, const srb_sim *dev_io, int cycle, void *stream);
int srb_rollout_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim, int cycles,
                       void *stream);

/*
 * Moving obstacles (LIP mode; DESIGN.md 3 "Moving obstacles", 10.6): an optional velocity per obstacle row, read by
 * the selection, the solve and the rollout.  The layouts of srb_batch and srb_sim (and SRB_ABI_VERSION) stay; the new
 * members travel in a struct of their own through entry points of their own, which otherwise behave as the entry
 * points they extend.
 *   obs_vel   [n_obs][2]    in: row i is the velocity (m/s) of obstacles[i]; row order and, with scenes, the
 *                           scene-major layout of `obstacles` (scene g owns rows [g scene_obs, + scene_obs) of both
 *                           tables).  The static column j < K_obs of grid k of the NLP stage then reads
 *                               o = obstacles[sel[j]] + obs_vel[sel[j]] * (Ts * (k + 1))
 *                           (uncontracted) where it read obstacles[sel[j]]; the table is read only through sel.
 *                           NULL: static obstacles.
 *   horizon_selection       0: the K_obs static columns are the rows nearest now (srb_knn_kernel, as ever);
 *                           1: the rows of closest predicted approach over the horizon
 *                           (srb_knn_obs_horizon_kernel): the key of row i for an agent is
 *                           sqrt(min over k = 0 .. N of dx^2 + dy^2), t_k = Ts * (double)k, the agent at
 *                           (x0[0] + x0[1] t_k, x0[2] + x0[3] t_k) -- constant velocity even when a plan table is
 *                           present -- and the obstacle at (o_x + w_x t_k, o_y + w_y t_k), squares and sums
 *                           uncontracted, a NaN pair making the key NaN for good.  Order, lower index on ties,
 *                           never-selected NaN rows and the static table's 1000 m rule (a slot whose key is >= 1000
 *                           gets row 0, with scenes the scene's row 0) are those of the snapshot selection.  One
 *                           workgroup per agent, brute force: no selection grid is built or consulted.  The
 *                           neighbour columns are selected as ever, by the snapshot or by plans.  Needs obs_vel.
 *   obstacles [n_obs][2]    srb_rollout_moving_device only: the table the driver moves in place -- the rows
 *                           batch.obstacles points to, writable.
 * With mv == NULL or mv->obs_vel == NULL each entry point is the entry point it extends, output bits included.
 * SRB_ERR_ARG, by name and before anything is launched: a wrong struct_size; obs_vel together with
 * batch.obstacles_version != 0 (a kept selection grid of a moving table is stale); horizon_selection without obs_vel;
 * a rollout with obs_vel but without mv->obstacles, or whose mv->obstacles is not batch.obstacles.  Scenes and
 * agent_offset shards are honoured exactly as by the entry points extended.  host_mv holds host pointers, mv device
 * pointers.
 *
 * srb_select_moving_device: srb_select_device; with horizon_selection = 1, tables & 1 is the horizon-aware obstacle
 * selection.  The solve entry points run that selection themselves when horizon_selection = 1 (SRB_OPT_SELECTION = 1).
 *
 * srb_obstacles_advance_device(ctx, n_obs, obstacles, obs_vel, stream): one control cycle (NDOMAIN = 4 grids) of the
 * table, one thread per row (srb_obstacles_advance_kernel), uncontracted:
 *     obstacles[i][d] = obstacles[i][d] + obs_vel[i][d] * (Ts * 4.0)
 * No bounce and no interaction between obstacles.
 *
 * srb_rollout_moving_device: srb_rollout_device with the table moved.  For each cycle c it enqueues the agents'
 * advance; for c > c_first the obstacle advance; the metrics (unchanged: they read the moved table, so d_obs and
 * fail_cycle are taken at matching times); select + solve with the table; and after the last cycle the final flushing
 * advance of the agents.  Plain launches, no host synchronisation; plans on or off exactly as srb_rollout_device.
 * The SRB-12 mode takes the same struct through srb12_*_moving* entry points of its own (below, after srb12_plans); the
 * MPC_dist shims have no moving obstacles.
 */
typedef struct srb_moving {
    int struct_size;           /* sizeof(srb_moving) (ABI check) */
    const double *obs_vel;     /* [n_obs][2]; NULL: static obstacles */
    int horizon_selection;     /* 0: K_obs nearest now; 1: closest predicted approach over the horizon */
    double *obstacles;         /* advance / rollout only: the table moved in place (the rows batch.obstacles points to) */
} srb_moving;
int srb_solve_batch_moving(srb_ctx *ctx, int n_agents, const srb_batch *host_io, const srb_moving *host_mv);
int srb_solve_batch_moving_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv, void *stream);
int srb_select_moving_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv, int tables,
                             void *stream);
int srb_obstacles_advance_device(srb_ctx *ctx, int n_obs, double *obstacles, const double *obs_vel, void *stream);
int srb_rollout_moving_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim,
                              const srb_moving *mv, int cycles, void *stream);

/*
 * Obstacle sizes (LIP mode; DESIGN.md 3 "Obstacle sizes", 10.8): an optional CBF level and an optional body radius per
 * obstacle row.  As with srb_moving, the layouts of srb_batch, srb_sim and srb_moving (and SRB_ABI_VERSION) stay: the
 * tables travel in a struct of their own through entry points of their own, each of which takes the srb_moving of the
 * entry point it extends (mv may be NULL) and otherwise behaves as that entry point.
 *   obs_eps    [n_obs]      in: the CBF level of obstacles[i] in squared metres, the unit of srb_params.eps_obs: the
 *                           row of static column j at grid k reads  -|p_k - o_kj|^2 - s <= -obs_eps[sel[j]].  Row
 *                           order and, with scenes, the scene-major layout of `obstacles`.  The table is read only
 *                           through sel; the neighbour columns and a -1 row keep eps_nbr.  NULL: eps_obs for every row.
 *   obs_radius [n_obs]      in: the body radius (m) of obstacles[i] for the metrics' fail test: d_obs is then
 *                           min over i of (dist_i - obs_radius[i]) (one rounded subtract; a NaN term never wins; an
 *                           empty table gives +inf), fail_cycle the first cycle with d_obs < 0; min_d_obs,
 *                           distance_to_fail and the agent-to-agent outputs follow the rules of srb_sim.  A uniform
 *                           0.5 table gives srb_sim's d_obs - 0.5 bit for bit and its fail_cycle.  NULL: the metrics
 *                           of srb_sim (centre distances, 0.5 m).
 *   clearance_selection     0: the K_obs static columns as ever (nearest centres now, or with
 *                           srb_moving.horizon_selection the closest predicted approach);
 *                           1: by clearance to the level set (srb_knn_obs_clear_kernel): the key of row i for an
 *                           agent is sqrt(m) - sqrt(obs_eps[i]), uncontracted, m the squared distance now -- or, with
 *                           horizon_selection = 1, the min over k = 0 .. N of srb_knn_obs_horizon_kernel's squared
 *                           distances.  Keys may be negative (an agent inside a level set).  Order by key, lower index
 *                           on ties; a NaN key (a NaN row, a NaN or negative obs_eps) is never selected; a slot whose
 *                           key is >= 1000, or with no row left, gets row 0 (with scenes the scene's row 0).  One
 *                           workgroup per agent, brute force: no selection grid is built or consulted.  The neighbour
 *                           columns are selected as ever.  Needs obs_eps.
 * With sz == NULL, or every member NULL / 0, each entry point is the _moving entry point it extends, output bits
 * included.  SRB_ERR_ARG, by name and before anything is launched: a wrong struct_size; clearance_selection other than
 * 0 or 1; clearance_selection = 1 without obs_eps.  obs_eps goes together with obstacles_version != 0 (sizes do not
 * stale a grid of centres).  The QP-only solve ignores the tables.  host_sz holds host pointers, sz device pointers.
 *
 * srb_select_sized_device: with clearance_selection = 1, tables & 1 is the clearance selection.  The solve entry
 * points run it themselves (SRB_OPT_SELECTION = 1).  srb_sim_metrics_sized_device: srb_sim_metrics_device with
 * obs_radius.  srb_rollout_sized_device: srb_rollout_moving_device's sequence per cycle with the sized metrics, select
 * and solve; the tables do not change over a rollout.  The SRB-12 mode takes the same struct through srb12_*_sized*
 * entry points of its own (below, after the srb12_*_moving block); the MPC_dist shims have no obstacle sizes.
 */
typedef struct srb_sizes {
    int struct_size;            /* sizeof(srb_sizes) (ABI check) */
    const double *obs_eps;      /* [n_obs]: the CBF level of obstacles[i], squared metres, the unit of eps_obs; NULL: eps_obs for every row */
    const double *obs_radius;   /* [n_obs]: body radius (m) for the metrics' fail test; NULL: today's metrics */
    int clearance_selection;    /* 0: the K_obs columns as ever; 1: by clearance to the level set */
} srb_sizes;
int srb_solve_batch_sized(srb_ctx *ctx, int n_agents, const srb_batch *host_io, const srb_moving *host_mv,
                          const srb_sizes *host_sz);
int srb_solve_batch_sized_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                                 const srb_sizes *sz, void *stream);
int srb_select_sized_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                            const srb_sizes *sz, int tables, void *stream);
int srb_sim_metrics_sized_device(srb_ctx *ctx, int n_agents, const srb_sim *sim, const srb_sizes *sz, int cycle,
                                 void *stream);
int srb_rollout_sized_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim,
                             const srb_moving *mv, const srb_sizes *sz, int cycles, void *stream);

/*
 * Agent sizes (LIP mode; DESIGN.md 3 "Agent sizes", 10.10): an optional safety radius, pad and body radius per agent,
 * so that a mixed team (large carriers among small scouts) need not inflate every pair to the largest.  As with
 * srb_sizes, SRB_ABI_VERSION and the layouts of srb_batch, srb_sim, srb_moving and srb_sizes stay: the tables travel
 * in a struct of their own through entry points of their own, each of which takes the srb_moving and srb_sizes of
 * the _sized entry point it extends (both may be NULL) and otherwise behaves as that entry point.  Every table has
 * n_all rows in the row order of nbr_state (scene-major with scenes); global agent g = agent_offset + a owns row g.
 * The tables are read through sel and at row g only.  All arithmetic is fp64, uncontracted.
 *   agent_rad  [n_all]      in: safety radius (m).  The level of neighbour column j (K_obs <= j < K, sel[j] >= 0) is
 *                           s * s with s = agent_rad[g] + agent_rad[sel[j]] (one rounded add, one rounded multiply);
 *                           a -1 column keeps eps_nbr.  NULL: eps_nbr for every neighbour column.
 *   agent_pad  [n_all]      in: metres added to the safety radius of every static column of agent g: the level of
 *                           column j < K_obs becomes t * t with t = sqrt(e_j) + agent_pad[g], e_j the level the column
 *                           has after the obs_eps gather (eps_obs, or obs_eps[sel[j]]); sqrt correctly rounded.
 *                           May be negative.  NULL: the levels as they are.
 *   agent_body [n_all]      in: body radius (m), metrics only: d_agent is then
 *                           min over i != g of (sqrt(d2_i) - (agent_body[g] + agent_body[i])), d2_i the squared centre
 *                           distance of the metrics, the sum of the radii one rounded add; a NaN term never wins; a
 *                           table without another row gives +inf.  min_d_agent follows as ever.  A uniform table b
 *                           gives srb_sim's d_agent - (b + b) bit for bit.  The obstacle half (d_obs, fail_cycle,
 *                           distance_to_fail) is srb_sizes.obs_radius's when that table is given, else srb_sim's, and
 *                           does not look at agent bodies.  NULL: the metrics of the _sized call.
 *   clearance_selection     0: the K_nbr neighbour columns as ever (nearest centres now, or with
 *                           SRB_OPT_PLAN_SELECTION = 1 the closest predicted approach);
 *                           1: by clearance (srb_knn_nbr_clear_kernel): the key of row i is dist_i - agent_rad[i]
 *                           (the agent's own radius shifts every key alike and is left out), dist_i the snapshot
 *                           distance sqrt(dx*dx + dy*dy) -- or, with SRB_OPT_PLAN_SELECTION = 1 and a plan table,
 *                           sqrt(m), m the horizon-aware selection's minimum over the N + 1 pairs.  Keys may be
 *                           negative.  Order by key, lower index on ties; a NaN key is never selected; row g is left
 *                           out; a slot with no row left gets -1 (no 1000 m rule).  One workgroup per agent, brute
 *                           force: no selection grid is built or consulted.  The static columns are selected as
 *                           ever (centres, horizon or obstacle clearance).  Needs agent_rad.
 *   collide_cycle [A]       out, optional: the first cycle with d_agent < 0, else -1; set by the call with
 *                           cycle == c_first and never overwritten once set (fail_cycle's rules).  Needs agent_body.
 * With ag == NULL, or every member NULL / 0, each entry point is the _sized entry point it extends, output bits
 * included.  SRB_ERR_ARG, by name and before anything is launched: a wrong struct_size; clearance_selection other than
 * 0 or 1; clearance_selection = 1 without agent_rad; agent_rad or agent_body with a batch that has no neighbour table;
 * collide_cycle without agent_body.  The QP-only solve ignores the tables.  host_ag holds host pointers (agent_rad and
 * agent_pad are staged; agent_body and collide_cycle are not read by a solve), ag device pointers.
 * srb_rollout_agents_device refuses a shard, as srb_rollout_device does; the tables do not change over a rollout.
 * The SRB-12 mode takes the same struct through srb12_*_agents* entry points of its own (below, after the
 * srb12_*_sized block); the MPC_dist shims have no agent sizes.
 */
typedef struct srb_agent_sizes {
    int struct_size;            /* sizeof(srb_agent_sizes) (ABI check) */
    const double *agent_rad;    /* [n_all] safety radius (m) of table row i (the row order of nbr_state) */
    const double *agent_pad;    /* [n_all] metres added to the safety radius of every static column of agent i */
    const double *agent_body;   /* [n_all] body radius (m), metrics only */
    int clearance_selection;    /* 0: neighbour columns as ever; 1: by clearance (needs agent_rad) */
    int *collide_cycle;         /* [A] out, optional, metrics / rollout only */
} srb_agent_sizes;
int srb_solve_batch_agents(srb_ctx *ctx, int n_agents, const srb_batch *host_io, const srb_moving *host_mv,
                           const srb_sizes *host_sz, const srb_agent_sizes *host_ag);
int srb_solve_batch_agents_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                                  const srb_sizes *sz, const srb_agent_sizes *ag, void *stream);
int srb_select_agents_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                             const srb_sizes *sz, const srb_agent_sizes *ag, int tables, void *stream);
int srb_sim_metrics_agents_device(srb_ctx *ctx, int n_agents, const srb_sim *sim, const srb_sizes *sz,
                                  const srb_agent_sizes *ag, int cycle, void *stream);
int srb_rollout_agents_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim,
                              const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, int cycles,
                              void *stream);

/*
 * Disturbed plant (LIP mode; DESIGN.md 3 "Disturbed plant", 9, 10.12): kicks, pushes and a plant whose CoM height is
 * not the model's, so that a rollout can say whether the safety rows hold when the robot is shoved, its velocity is
 * noisy or the model is wrong.  As with srb_agent_sizes, SRB_ABI_VERSION and every existing struct stay: the tables
 * travel in a struct of their own through entry points of their own, which extend srb_sim_advance_device and
 * srb_rollout_agents_device (mv, sz, ag may be NULL) and otherwise behave as those.  Every table has n_all rows in
 * the row order of nbr_state (scene-major with scenes); global agent g = agent_offset + a owns row g (srb_sim's
 * agent_offset / n_all; n_all == 0 reads as n_agents rows).  All pointers are device pointers.  All arithmetic is
 * fp64, uncontracted, with one stated grouping (csrc/srb_plant.hip; tests/plant_oracle.py restates it bit for bit).
 *
 * The plant acts in the advance of a cycle c > c_first (at c_first the state is the caller's, as ever) and replaces
 * "state = x[a][12..15]" by state = z + d, one rounded add per component:
 *   z, the base state
 *     plant_hcom NULL       x[a][12..15], the nominal prediction.
 *     plant_hcom [n_all]    the four-step roll z <- Ad_g z + Bd_g u of the plant's own LIP, from the state that
 *                           started cycle c - 1 -- read from `state` before it is overwritten, so this advance is
 *                           NOT idempotent: call it once per cycle -- under the four inputs the model applied over
 *                           the domain, u = (x[4N + 2k], x[4N + 2k + 1]) for k = 0 .. 3 (the U_k of the equality row
 *                           X_k = Ad X_{k-1} + Bd U_k).  Ad_g, Bd_g are computed on the device from
 *                           grav / plant_hcom[g] and Ts by the arithmetic of the library's own discretisation (the
 *                           third-order series for Ad, A^-1 (Ad - I) B for Bd), operation for operation.  Each
 *                           matrix-vector product is a row sum in index order: Ad's four terms, then Bd's two.
 *   d = (dpx, dvx, dpy, dvy), the disturbance, from +0.0
 *     kick_v, kick_p [n_all]  bounds (m/s, m) of a uniform kick per cycle.  Philox4x32-10 with key
 *                           ((uint32)seed, (uint32)(seed >> 32)) and counter ((uint32)c, (uint32)g, 0, 0) gives
 *                           words w0 .. w3, and u_i = ((double)(int32_t)w_i + 0.5) * 2^-31 lies in (-1, 1), is
 *                           never 0 and is exact.  dvx += kick_v[g] u0, dvy += kick_v[g] u1, dpx += kick_p[g] u2,
 *                           dpy += kick_p[g] u3, each one rounded multiply and one rounded add.  Bounded and
 *                           uniform on purpose: a CBF margin is stated against a bounded disturbance.  The counter
 *                           holds the caller's cycle number c (not c - c_first) and the global row g (not a), so a
 *                           shard, a scene and a rollout continued cycle by cycle draw what the whole team draws in
 *                           one rollout call.
 *     pushes                every entry p, in table order, with push_cycle[p] == c and push_agent[p] == g adds
 *                           push_dv[p] to (dvx, dvy), one rounded add each, after the kick.  Brute force per agent.
 *                           An entry whose cycle is <= c_first, or is never reached, does not fire.
 *   dist_log [T][A][4]      out, optional: row c - c_first - 1 gets d.
 * Everything an advance derives from the state -- x0, last_state, alpha_buf, the reference, the footholds, the traj
 * row -- follows from the new state; the plan shift and the logs of the previous solve are unchanged, so a
 * neighbour's shifted plan is stale by the disturbance, as it would be on a robot.
 *
 * With plant == NULL, or every table NULL and n_push == 0, each entry point is the one it extends, output bits
 * included (dist_log is then not written).  SRB_ERR_ARG, by name, before anything is launched and before a context is
 * needed: a wrong struct_size; n_push outside 0 .. 4096; n_push > 0 with push_cycle, push_agent or push_dv missing;
 * plant_hcom with srb_sim.x missing (the advance; the rollout reads batch.x).  With a context: agent_offset +
 * n_agents beyond n_all.  The contents of the tables are NOT checked: a NaN or negative bound or height goes
 * through the arithmetic above as it is.  srb_rollout_plant_device refuses a shard, as srb_rollout_device does; the
 * tables do not change over a rollout.  The SRB-12 mode has a plant of its own (srb12_plant, below); the MPC_dist shims
 * have none.
 */
typedef struct srb_plant {
    int struct_size;            /* sizeof(srb_plant) (ABI check) */
    unsigned long long seed;    /* the Philox key */
    const double *kick_v;       /* [n_all] m/s bound per cycle, or NULL */
    const double *kick_p;       /* [n_all] m bound per cycle, or NULL */
    const double *plant_hcom;   /* [n_all] the plant's CoM height (m), or NULL: the nominal prediction */
    int n_push;                 /* 0 .. 4096 */
    const int *push_cycle, *push_agent;   /* [n_push]; agent = global row */
    const double *push_dv;      /* [n_push][2] m/s */
    double *dist_log;           /* [T][A][4] out, optional */
} srb_plant;
int srb_sim_advance_plant_device(srb_ctx *ctx, int n_agents, const srb_sim *sim, const srb_plant *plant, int cycle,
                                 void *stream);
int srb_rollout_plant_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim,
                             const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                             const srb_plant *plant, int cycles, void *stream);

/*
 * Degraded neighbour link (LIP mode; DESIGN.md 3 "Degraded link", 9, 10.14): what an agent knows about its neighbours
 * is late, lossy and noisy, so that a rollout can say whether the inter-agent CBF rows keep separation when snapshots
 * are cycles old, broadcasts are lost or positions are off by centimetres.  As with srb_plant, SRB_ABI_VERSION and
 * every existing struct stay.  The solve and its selection read the PERCEIVED tables seen_state / seen_plan; the
 * metrics, traj and every log keep reading the truth.  All pointers are device pointers; every table has n_all rows
 * in the row order of nbr_state, global row g.  All arithmetic is fp64, uncontracted, with one stated grouping
 * (csrc/srb_link.hip; tests/link_oracle.py restates it bit for bit).
 *
 * One broadcast per agent per cycle, and every receiver sees the same fate of a message (a per-sender model: the
 * perceived tables keep n_all rows).  At every cycle s >= c_first row g sends its snapshot row last_state[g]
 * (x, y, xdot, ydot) and, for s > c_first with a plan table, its shifted plan plan_table[g] [N][2].
 *   noise_p, noise_v [n_all]  at the sender: Philox4x32-10 with key ((uint32)seed, (uint32)(seed >> 32)) and counter
 *                         ((uint32)s, (uint32)g, 3, 0) gives w0 .. w3, u_i = ((double)(int32_t)w_i + 0.5) * 2^-31, and
 *                         the message's state is (x + noise_p[g] u0, y + noise_p[g] u1, xdot + noise_v[g] u2,
 *                         ydot + noise_v[g] u3), each one rounded multiply and one rounded add.  A NULL table leaves its
 *                         components untouched (it does not add 0.0).  Plans carry no noise.
 *   drop [n_all]          message (s, g) is lost iff s > c_first and 0.5 * u0 + 0.5 < drop[g], u0 from the counter
 *                         ((uint32)s, (uint32)g, 2, 0).  The left side is exact and inside (0, 1): 0 never loses, 1
 *                         always does.  The message of c_first is never lost and arrives at once.
 *                         (srb_plant draws with third counter words 0 and 1: one seed may serve both.)
 *   delay [n_all] int     0 .. max_delay cycles (NULL: 0), clamped into that range by the kernel; max_delay <= 16.
 *                         The message of cycle s is kept in slot (s - c_first) mod (max_delay + 1) of the ring.  At
 *                         cycle c > c_first the message of s = c - delay[g] arrives if s > c_first and it was not lost:
 *                         it becomes the held message and held_cycle[g] = s.  Otherwise the receiver keeps what it
 *                         holds.  age = c - held_cycle[g].
 *   extrapolate           0: seen_state[g] / seen_plan[g] are the held state / plan as they are.  1: the receiver
 *                         dead-reckons: position + velocity * ((double)(4 age) * Ts), velocities as held, and the held
 *                         plan shifted by 4 age grids with the rule of srb_sim.plan_table: grid k is the held grid
 *                         k + 4 age while that lies inside the horizon, beyond it
 *                         last + (double)(k + 4 age - N + 1) * (last - previous); age 0 is a copy of both.
 *   With either setting a row that holds no plan yet (held_cycle == c_first) at a cycle c > c_first with a plan table
 *   gets the constant-velocity line from its SEEN state, p + v * (Ts * (double)(k + 1)).  At c_first no plan is sent
 *   and seen_plan, held_plan and ring_plan are not written: the first solve reads batch.nbr_plan as ever.
 *   age_log [T][n_all] int  out, optional: row c - c_first gets age.
 * The draws key on the caller's cycle number and the global row, so a shard, a scene replica and a rollout continued
 * cycle by cycle draw what the whole team draws in one call.
 *
 * srb_link_update_device(ctx, n_all, link, last_state, plan_table, cycle, c_first, stream): the update of one cycle
 * (srb_link_update_kernel), always over all n_all rows -- every shard computes the whole perceived table itself from the
 * gathered truth (last_state [n_all][4], plan_table [n_all][N][2] or NULL).  Call it once per cycle, from c_first on,
 * with the same max_delay throughout.  Asynchronous on `stream`, ordered by the context like the other device calls.
 * srb_rollout_link_device extends srb_rollout_plant_device (which is this call with link == NULL): after the metrics
 * of every cycle the update runs on sim.last_state / sim.plan_table, the solve reads link->seen_state as its nbr_state
 * and, from the second cycle with a plan table, link->seen_plan as its nbr_plan.
 *
 * A link is on when any of delay, drop, noise_p, noise_v is set.  With link == NULL or all four NULL nothing is
 * launched and every output has the bits it had (age_log then stays unwritten).  SRB_ERR_ARG, by name, before anything
 * is launched and before a context is needed: a wrong struct_size; max_delay outside 0 .. 16; extrapolate not 0 / 1; a
 * link that is on without ring_state, held_state, held_cycle or seen_state; a plan table without ring_plan, held_plan
 * or seen_plan; seen_state overlapping last_state.  With a context (the ranges need N): seen_plan overlapping
 * plan_table or batch.plan; SRB_OPT_PLAN_SELECTION = 1 with a link on (that selection reads the agent's own previous
 * plan from its row of the table, which would be a stale copy of what the agent knows exactly: not built); a shard in
 * the rollout driver, as ever.  The contents of the tables are NOT checked otherwise.  That refusal of the plan selection
 * is the LIP mode's and stays as it is; the SRB-12 mode has the link with the selection (srb12_rollout_link_device
 * below), whose own plan comes from the truth.  The MPC_dist shims have no link.
 */
typedef struct srb_link {
    int struct_size;            /* sizeof(srb_link) (ABI check) */
    unsigned long long seed;    /* the Philox key */
    const int *delay;           /* [n_all] cycles, 0 .. max_delay, or NULL */
    const double *drop;         /* [n_all] loss probability per message, or NULL */
    const double *noise_p;      /* [n_all] m bound on the sent position, or NULL */
    const double *noise_v;      /* [n_all] m/s bound on the sent velocity, or NULL */
    int max_delay;              /* 0 .. 16: the ring holds max_delay + 1 cycles */
    int extrapolate;            /* 0 / 1 */
    double *ring_state;         /* [(max_delay + 1)][n_all][4]     caller-owned state of the link ... */
    double *ring_plan;          /* [(max_delay + 1)][n_all][N][2] */
    double *held_state;         /* [n_all][4] */
    double *held_plan;          /* [n_all][N][2] */
    int *held_cycle;            /* [n_all] */
    double *seen_state;         /* [n_all][4] out: the perceived snapshot table */
    double *seen_plan;          /* [n_all][N][2] out: the perceived plan table */
    int *age_log;               /* [T][n_all] out, optional */
} srb_link;
int srb_link_update_device(srb_ctx *ctx, int n_all, const srb_link *link, const double *last_state,
                           const double *plan_table, int cycle, int c_first, void *stream);
/* the same update by a stated thread mapping, for tools/bench_link.py and the tests: lanes threads per row, 1, 8 or 16
 * (srb_link_update_device uses the measured choice); every mapping gives the same bits */
int srb_link_update_lanes_device(srb_ctx *ctx, int n_all, const srb_link *link, const double *last_state,
                                 const double *plan_table, int cycle, int c_first, int lanes, void *stream);
int srb_rollout_link_device(srb_ctx *ctx, int n_agents, const srb_batch *dev_io, const srb_sim *sim,
                            const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                            const srb_plant *plant, const srb_link *link, int cycles, void *stream);

/*
 * HL reference planner (generateReferenceTrajectory, MPC_dist.cpp:930-1104; SURVEY.md 8(f)
 * row 3) on HIP device `device`, host buffers, synchronous.  NA agents (1..2^20; up to 1024 in
 * one persistent workgroup, more -- one coupled swarm -- as one launch per step) starting at
 * Pstart [NA][2], planner obstacles Pobs [n_obs][2] (n_obs <= 2048), `loop` steps (reference:
 * 100000).  Outputs Pr_refined_ / Prd_refined_ as column-major 2NA x (loop / 40) arrays (the
 * layout setReferenceTrajectory / srb_prep take).  Returns 0 or a negative error code.
 */
int srb_hl_plan(int device, int NA, const double *Pstart, const double *Pobs, int n_obs, int loop, double *Pr,
                double *Prd);

/* Per-launch timing of the last srb_solve_batch_device call, measured with HIP events on
 * the stream the kernel ran on (ms): knn_ms the obstacle / neighbour selection kernel
 * (0 when nothing is selected: QP only, or K_obs = K_nbr = 0), solve_ms the solve kernel. */
int srb_last_kernel_ms(srb_ctx *ctx, float *knn_ms, float *solve_ms);
/* ... and of the active-set polish of the NLP result (srb_polish_kernel, launched right after the
 * solve kernel), ms. */
int srb_last_polish_ms(srb_ctx *ctx, float *polish_ms);

/* Dynamic LDS bytes one agent's workgroup uses (for occupancy reports). */
int srb_lds_bytes(const srb_params *p);

/* Bezier fit of the predicted CoM states (fitComTrajectory_eventbase, MPC_dist.cpp:784-855),
 * host-side: alpha[4][5] from the buffer state buf[4] and X[0..3] (4 states). */
void srb_fit_bezier(const double buf[4], const double *X, double alpha[20]);

/*
 * ---- Low-level CLF-QP controller ----------------------------------
 * Replaces LowLevelCtrl::calcTorque(state, dyn, kin, vc, con, params)
 * (/root/reference/include/LowLevelCtrl.hpp:20, src/LowLevelCtrl.cpp:18-113) for a batch of
 * agents: QP assembly (cost :115-137, constraints :139-236), the iswiftQp_e solve (:33-37,
 * iSWIFT Prime.c:127-230), the parse into ll.QP_force / tau / dV (:44-64), swing-leg PD
 * (:71-91), the integration ll.ddq / ll.dq / ll.q (:96-98) and swingInvKin (:446-488).
 * One QP per agent: numDec = 3c + 12 + outDim + useCLF (<= 31) variables
 * [F (3c, stance legs FR,FL,RR,RL) | tau (12) | aux (outDim = 6 + 3(4-c)) | d].
 */
typedef struct srb_ll_params {      /* Settings::LL_params (global_loco_structs.hpp:96-111) */
    double mu, kp, kd;
    int useCLF;
    double tauPen, dfPen, auxPen, clfPen, auxMax, clfEps;
    int maxit;                      /* iSWIFT MAXIT 25 (GlobalOptions.h:23) */
    double tol;                     /* 1e-6 (GlobalOptions.h:24-25) */
} srb_ll_params;

/* Parameters.cpp:62-75 defaults: mu 0.7, kp 700, kd 40, useCLF 1, tauPen 1, dfPen 0.1,
 * auxPen 1e6, clfPen 1e8, auxMax 100, clfEps 0.8. */
void srb_ll_params_default(srb_ll_params *p);

/*
 * One batch, agent-major.  Matrices are column-major (Eigen's storage) with FIXED leading
 * dimensions, so every agent has the same stride whatever its contact count:
 *   ind      [A][4] int      ConInf::ind (1 stance, 0 swing; other values -> status 3)
 *   q, dq    [A][18]         StateInfo::q, dq
 *   Dinv     [A][18*18]      DynamicsInfo::Dinv
 *   B        [A][12*18]      DynamicsInfo::B (18 x 12, ld 18)
 *   H        [A][18]         DynamicsInfo::H
 *   Jc, Js   [A][18*12]      KinematicsInfo::Jc (3c x 18), Js ((12-3c) x 18), ld 12
 *   dJc      [A][12]         KinematicsInfo::dJc (3c used)
 *   Jtoe, Jhip [A][18*12]    KinematicsInfo::Jtoe, Jhip (12 x 18, ld 12)
 *   toePos, hipPos [A][12]   KinematicsInfo::toePos, hipPos (3 x 4: column per leg)
 *   H0       [A][18*18]      VCInfo::H0 (outDim x 18, ld 18)
 *   dH0, y, dy [A][18]       VCInfo (outDim used)
 *   hd, dhd  [A][18]         VCInfo::hd, dhd (rows 6.. hold the swing-toe targets)
 *   fDes     [A][12]         VCInfo::fDes
 * In/out:
 *   tau      [A][18]         LowLevelCtrl::tau (the member array: entries 0..5 carry over
 *                            between calls and accumulate the swing PD, :91)
 * Outputs:
 *   QP_force [A][12], ddq, dq_out, q_out [A][18]  LLInfo (global_loco_structs.hpp:74-80)
 *   V, dV    [A]             LLInfo::V, dV
 *   x        [A][32]         QP solution (optimOut), zero-padded beyond numDec; may be NULL
 *   status   [A] int         iSWIFT exit code (0 OPTIMAL, 1 KKTFAIL, 2 MAXIT, 3 bad contact flags)
 *   iters    [A] int         interior-point iterations
 */
typedef struct srb_ll_io {
    int struct_size;         /* sizeof(srb_ll_io) (ABI check) */
    const int *ind;
    const double *q, *dq, *Dinv, *B, *H, *Jc, *dJc, *Js, *Jtoe, *Jhip, *toePos, *hipPos;
    const double *H0, *dH0, *y, *dy, *hd, *dhd, *fDes;
    double *tau, *QP_force, *ddq, *dq_out, *q_out, *V, *dV, *x;
    int *status, *iters;
} srb_ll_io;

typedef struct srb_ll_ctx srb_ll_ctx;

int srb_ll_ctx_create(const srb_ll_params *p, int max_agents, int device, srb_ll_ctx **out);
int srb_ll_ctx_destroy(srb_ll_ctx *ctx);
/* host buffers: copies in, solves, copies out, synchronises */
int srb_ll_calc_torque(srb_ll_ctx *ctx, int n_agents, const srb_ll_io *host_io);
/* device buffers, asynchronous on `stream` (NULL = the HIP null stream); call srb_ll_sync() */
int srb_ll_calc_torque_device(srb_ll_ctx *ctx, int n_agents, const srb_ll_io *dev_io, void *stream);
int srb_ll_sync(srb_ll_ctx *ctx);
/* HIP-event time of the last srb_ll_calc_torque[_device] kernel on its stream (ms) */
int srb_ll_last_kernel_ms(srb_ll_ctx *ctx, float *ms);

/* ================================================================ SRB-12 extension mode
 * The north star's 12-state single-rigid-body NMPC (state [p, roll/pitch/yaw, v, omega], inputs the
 * four leg forces, friction pyramid + f_z <= fmax, the obstacle rows of the LIP mode).  The
 * reference DECLARES this solver (FastMPC::runMPC / MPC_Cost / MPC_Constraints /
 * getLinearDynamics, include/fast_MPC.hpp:98-103) without implementing it, so these entry points
 * replace no reference binding; the problem is stated in DESIGN.md section 11, the CPU checker is
 * oracle/srb12.c (parity with the reference unpinned).  Constants: mass and inertia of FastMPC
 * (src/fast_MPC.cpp:40-43), weights and mu_MPC of the default mpc_params (src/Parameters.cpp:32-52).
 */
typedef struct srb12_params {
    int N, K_obs, K_nbr;          /* grids (<= 24), nearest static obstacles / neighbours (each <= 16) */
    double Ts, mass, Ib[9], grav, mu, fmax;
    double q[12], qN[12], r[3], Sw;     /* stage / terminal state weights, force weights (per axis), slack */
    double eps_obs, eps_nbr, tol;
    int qp_maxit, nlp_maxit, use_nlp;
    double z0;                    /* NLP initial duals z0 / max(s, 1) */
    double tol_final;             /* complementarity s'z/m < tol_final ends the LAST stage (the NLP, or the QP when
                                     use_nlp = 0; default 1e-8): far enough for the polish to identify the active
                                     set (without the polish 1e-8 leaves the forces up to 1e-3 N from
                                     the exact optimum, 1e-6 up to 3e-2 N) */
    int polish;                   /* 1 (default): the last stage's result is polished to the exact KKT point of
                                     its active set (forces within 1e-4 N of the optimum); 0 off */
    double tol_qp;                /* the QP stage's tolerance when the NLP stage follows it (default 1e-3; 0: tol):
                                     the NLP is warm-started from that point, so its accuracy does not carry into
                                     the result (QP iterations 4.1 -> 2.6 on average, 6 -> 4 at most) */
} srb12_params;

void srb12_params_default(srb12_params *p, int N);
int srb12_nv(const srb12_params *p);   /* 24N + 1: X = x_1..x_N (12N) | U = u_0..u_{N-1} (12N) | s */

/* Batch buffers, agent-major fp64 (int32 where noted):
 *   x0 [A][12]; xref [A][N][12] (x_1..x_N); foot [A][N][4][3] (world foot positions per grid, legs FR FL
 *   RR RL); contact [A][N][4] int (1 stance); obstacles / nbr_state / n_obs / n_all / agent_offset /
 *   sel / obstacles_version as in srb_batch (the neighbour snapshot rows are [x, y, xdot, ydot]);
 *   outputs x_qp (may be NULL), x [A][24N+1], obj [A], status [A][2], iters [A][2]; a FATAL (3) QP stage ends the
 *   solve before the NLP stage, whose status then reads FATAL as well (use_nlp = 1).
 *   status codes 0..3 as iSWIFT's; 4 by stage: the LAST stage (the NLP, or the QP when use_nlp = 0) converged but
 *   its polish was rejected (the interior-point result is returned); the QP stage followed by the NLP converged at
 *   tol_qp only (QP_WARM, x_qp is the NLP's warm start); with use_nlp = 0 status[1] and iters[1] read 0 */
typedef struct srb12_batch {
    int struct_size;              /* sizeof(srb12_batch) (ABI check) */
    const double *x0, *xref, *foot;
    const int *contact;
    const double *obstacles, *nbr_state;
    int n_obs, n_all, agent_offset;
    double *x_qp, *x, *obj;
    int *status, *iters;
    int *sel;                     /* optional [A][K_obs + K_nbr] selected rows */
    int obstacles_version;
} srb12_batch;

typedef struct srb12_ctx srb12_ctx;
int srb12_ctx_create(const srb12_params *p, int max_agents, int device, srb12_ctx **out);
int srb12_ctx_destroy(srb12_ctx *ctx);
/* host buffers: copies in, solves, copies out, synchronises */
int srb12_solve_batch(srb12_ctx *ctx, int n_agents, const srb12_batch *host_io);
/* device buffers, asynchronous on `stream` (NULL = the HIP null stream) */
int srb12_solve_batch_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, void *stream);
/* HIP-event times of the last call's selection and solve kernels (ms) */
int srb12_last_kernel_ms(srb12_ctx *ctx, float *select_ms, float *solve_ms);
/* 1 (default): HIP events around the selection and solve kernels (srb12_last_kernel_ms); 0: none */
int srb12_ctx_set_timing(srb12_ctx *ctx, int on);
int srb12_lds_bytes(const srb12_params *p);
/* The solve kernel the last launch ran, by name (srb12_kernel_<TL>_<TO>_<NC>_<K1>, srb12_kernel_mv_* with a table):
 * static storage, written at the launch; "" before the first.  srb12_kernel_table / srb12_pick_kernel: the shipped
 * instances (dims TL, TO, NC, K1; SRB_ERR_ARG past the end) and the one that horizon N with K rows per grid picks
 * (SRB_ERR_SIZE where none fits); host only, as srb_kernel_table / srb_pick_kernel. */
int srb12_ctx_last_kernel(srb12_ctx *ctx, const char **solve);
int srb12_kernel_table(int i, int dims[4], const char **name);
int srb12_pick_kernel(int N, int K, int dims[4]);
/* The parameter checks of srb12_ctx_create alone (the 160 KiB LDS bound among them), host only. */
int srb12_check_params(const srb12_params *p);

/* Scenes in the SRB-12 mode: srb_ctx_set_scenes / srb_ctx_scenes forwarded to the context's selection.  The rules,
 * the per-call refusals and their messages are those of the LIP mode (see srb_ctx_set_scenes); they are honoured by
 * srb12_solve_batch, srb12_solve_batch_device, srb12_sim_metrics_device and srb12_rollout_device.  "Up to K nearest"
 * clamps to the agent's scene (K_obs to scene_obs, K_nbr to scene_agents - 1), and `sel` holds global row indices. */
int srb12_ctx_set_scenes(srb12_ctx *ctx, int scene_agents, int scene_obs);
int srb12_ctx_scenes(srb12_ctx *ctx, int *scene_agents, int *scene_obs);

/*
 * Closed-loop team rollout of the SRB-12 mode on the device: srb_sim's step and safety log for
 * the 12-state body.  One cycle is one gait domain of NDOMAIN = 4 grids, so N >= 4.  The plant of these entry points
 * is nominal (srb12_plant, further down, disturbs it through entry points of its own): the state
 * that starts cycle c + 1 is the X the solve of cycle c predicted at grid index 3, x[a][36..47], whatever that
 * solve's status.  All pointers are device pointers, fp64 unless noted; cycles count from c_first, and log rows are
 * indexed by c - c_first.
 *
 * srb12_sim_advance_device(ctx, A, sim, c, stream), cycle c >= c_first:
 *   state       [A][12]      p(3), roll/pitch/yaw(3), v(3), omega(3).  c == c_first: read (the caller's start
 *                            state); later cycles: written from x[a][36..47]
 *   goal        [A][2]       in: each agent's goal
 *   phase       [A] int      in, optional: added to c for the trot parity
 *   vref                     reference speed (the synthetic workload's: 0.27)
 *   hcom                     reference height of the CoM (the synthetic workload's: 0.3)
 *   yaw_step, hold_radius    the yaw reference: with e the bearing of the goal minus the yaw, wrapped to
 *                            [-pi, pi] (e -= 2 pi rint(e / 2 pi)) and clamped to +-yaw_step, yaw_ref = yaw + e
 *                            when the goal is farther than hold_radius, else the yaw itself.  A function of the
 *                            state alone, so a logged state reproduces it.  (Python defaults: 0.1 rad, the heading
 *                            offset workload.make_batch12 draws, and 0.05 m)
 *   gait                     0 trot, 1 stand
 *   x, status, iters         in: the previous solve's outputs (srb12_batch layout); x is required when c != c_first
 *   x0 [A][12], xref [A][N][12], foot [A][N][4][3], contact [A][N][4] int   out: the srb12_batch inputs of cycle c.
 *                            With d = goal - (x, y), dist = |d|, w = (d / dist) min(vref, dist / (Ts N)) (0 at the
 *                            goal: a standing reference that never overshoots) and t = Ts (k + 1), xref grid k is
 *                            columns 0, 1 = p + w t, 2 = hcom, 5 = yaw_ref, 6, 7 = w, every other column 0.  foot
 *                            grid k, domain j = k / 4: leg l (FR, FL, RR, RL) at centre + R(yaw_ref) STANCE[l], z = 0,
 *                            centre = p + w (Ts 4 j), STANCE the default stance (MPC_dist.cpp:1206-1209).  contact:
 *                            stand sets all four legs; trot {FR,RL} when c + phase + j is even, {FL,RR} when odd
 *   last_state  [A][4]       out: x, y, xdot, ydot -- the neighbour-snapshot row (get_lastState)
 *   com         [A][4]       out: x, xdot, y, ydot -- the row the selection and the metrics scan read
 *   traj        [T+1][A][12] out, optional: row c - c_first gets the state
 *   status_log, iters_log [T][A][2] int, x_log [T][A][24N+1]  out, optional, c != c_first only: row c - c_first - 1
 *                            gets the previous solve's status, iters, x
 * srb12_sim_metrics_device(ctx, A, sim, c, stream): the safety metrics of the `com` rows at the start of cycle c --
 * the kernels, the scan and the update rules of srb_sim_metrics_device, brute force and independent of the solver's
 * own selection:
 *   obstacles [n_obs][2], nbr_state [n_all][4], agent_offset   in: as in srb12_batch (row agent_offset + a is the
 *                            agent itself and is left out); either table may be empty
 *   d_obs, d_agent, min_d_obs, min_d_agent [A], fail_cycle [A] int, distance_to_fail [A]   out, optional: exactly
 *                            as in srb_sim (a NaN row never wins, an empty table gives +inf, the first cycle with
 *                            d_obs < 0.5 is kept); the running results are initialised by the call with c == c_first
 * Both are asynchronous on `stream` and ordered by the context like srb12_solve_batch_device.
 *
 * srb12_rollout_device(ctx, A, batch, sim, cycles, stream): `cycles` whole cycles of one team on one GPU.  For
 * c = c_first .. c_first + cycles - 1 it enqueues advance, metrics and solve, then one final advance that flushes
 * the last logs and the end state -- plain launches, no graph capture, no host synchronisation.  The two structs
 * are wired together here: the solve reads sim's x0, xref, foot, contact and sim.last_state as its nbr_state with
 * n_all = A, agent_offset = 0; the advance reads batch's x, status, iters; the metrics read batch's obstacles /
 * n_obs and sim.last_state.  The members of either struct that this replaces are ignored; batch.n_all /
 * agent_offset must be A / 0 or both 0 (a shard cannot roll out alone: its neighbours move too).  With scenes,
 * A must be a whole number of scenes.  This driver's solve has no nbr_plan input: the inter-agent rows use the
 * constant-velocity guess in every cycle.  srb12_rollout_plans_device (below) is the driver that feeds last
 * cycle's plans forward.
 */
typedef struct srb12_sim {
    int struct_size;         /* sizeof(srb12_sim) (ABI check) */
    double *state;
    const double *goal;
    const int *phase;
    double vref, hcom, yaw_step, hold_radius;
    int gait, c_first;
    const double *x;
    const int *status, *iters;
    double *x0, *xref, *foot;
    int *contact;
    double *last_state, *com;
    double *traj;
    int *status_log, *iters_log;
    double *x_log;
    const double *obstacles, *nbr_state;
    int n_obs, n_all, agent_offset;
    double *d_obs, *d_agent, *min_d_obs, *min_d_agent;
    int *fail_cycle;
    double *distance_to_fail;
} srb12_sim;
int srb12_sim_advance_device(srb12_ctx *ctx, int n_agents, const srb12_sim *dev_io, int cycle, void *stream);
int srb12_sim_metrics_device(srb12_ctx *ctx, int n_agents, const srb12_sim *dev_io, int cycle, void *stream);
int srb12_rollout_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim, int cycles,
                         void *stream);

/*
 * Neighbour plans in the SRB-12 mode: srb_batch.nbr_plan / plan and SRB_OPT_PLAN_SELECTION for the 12-state body.
 * The layouts of srb12_batch and srb12_sim stay; the plan pointers travel in a struct of their own through entry
 * points of their own, which otherwise behave as srb12_solve_batch[_device] / srb12_rollout_device do.
 *   nbr_plan  [n_all][N][2] in: row i, grid k is global agent i's predicted (x, y) at time (k+1) Ts from the
 *                           snapshot.  The neighbour rows of the NLP stage read it in place of the constant-
 *                           velocity guess p + v Ts (k+1); read only by the NLP stage and only for the neighbour
 *                           columns of `sel` (a -1 column keeps the no-neighbour row x0 + 1000 m).  Row
 *                           agent_offset + a is agent a's own previous plan: the horizon-aware selection reads
 *                           it, the CBF rows never do.  Needs nbr_state (the selection's snapshot); with scenes
 *                           the rows are scene-major like the snapshot.  NULL: constant velocity.
 *   plan      [A][N][2]     out: (X[12k], X[12k+1]) of the returned x for every agent, whatever its status (FATAL,
 *                           MAXIT and a rejected polish included); with use_nlp = 0 from the QP x.  Must not
 *                           overlap nbr_plan or plan_table.  NULL: not written.
 *   plan_selection          0: the neighbour columns are the rows nearest now (the snapshot selection);
 *                           1: the rows of closest predicted approach over the horizon (srb_knn_plan_kernel, with
 *                           scenes srb_knn_plan_scene_kernel on the agent's scene); needs nbr_plan.  The static
 *                           columns are selected as ever.
 *   plan_table [A][N][2]    srb12_rollout_plans_device only: the table of the next cycle (below).
 * A srb12_plans whose pointers are all NULL and whose plan_selection is 0 gives the bits of
 * srb12_solve_batch[_device].  SRB_ERR_ARG, before anything is launched: a wrong struct_size; nbr_plan without
 * nbr_state; K_nbr > 0 with agent_offset + n_agents > n_all; plan_selection = 1 without nbr_plan; plan == nbr_plan
 * or plan == plan_table.  host_plans holds host pointers, dev_plans device pointers.
 *
 * srb12_shift_plans_device(ctx, A, plan, grids, table, stream): last cycle's plans as this cycle's table, on the
 * device (srb12_plan_shift_kernel): the new cycle starts `grids` grids later, so table[a][k] = plan[a][k + grids]
 * for k < N - grids, and past the horizon last + m (last - previous), m = k + grids - N + 1.  grids >= 0, N >= 2;
 * plan and table [A][N][2] must be different buffers.
 *
 * srb12_rollout_plans_device(ctx, A, batch, sim, plans, cycles, stream): srb12_rollout_device with the plans fed
 * forward.  plans.plan and plans.plan_table are required.  The first solve reads plans.nbr_plan (NULL: constant
 * velocity); after every solve the shift (grids = 4, one gait domain) writes plan_table from plan, and every later
 * solve reads plan_table as its nbr_plan.  plan_selection applies to every cycle that has a table.  No host
 * synchronisation; scenes are honoured; a sharded batch is refused as by srb12_rollout_device.
 */
typedef struct srb12_plans {
    int struct_size;          /* sizeof(srb12_plans) (ABI check) */
    const double *nbr_plan;   /* [n_all][N][2]: row i, grid k = global agent i's (x, y) at Ts (k+1); NULL = constant velocity */
    double *plan;             /* [A][N][2] out: (X[12k], X[12k+1]) of the returned x; NULL = not written */
    int plan_selection;       /* 0: neighbours nearest now (snapshot); 1: closest predicted approach over the horizon */
    double *plan_table;       /* rollout only: [A][N][2] the table of the next cycle */
} srb12_plans;
int srb12_solve_batch_plans(srb12_ctx *ctx, int n_agents, const srb12_batch *host_io, const srb12_plans *host_plans);
int srb12_solve_batch_plans_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_plans *dev_plans,
                                   void *stream);
int srb12_shift_plans_device(srb12_ctx *ctx, int n_agents, const double *plan, int grids, double *table, void *stream);
int srb12_rollout_plans_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                               const srb12_plans *plans, int cycles, void *stream);

/*
 * Moving obstacles in the SRB-12 mode (DESIGN.md 3 "Moving obstacles", 10.7): srb_moving (above), its members with the
 * meaning they have in the LIP mode.  The static column j < K_obs of grid k of the NLP stage reads
 *     o = obstacles[sel[j]] + obs_vel[sel[j]] * (Ts * (k + 1))      (uncontracted, Ts of srb12_params)
 * through the srb12_kernel_mv_* instances; the -1 row and the neighbour columns (constant velocity or nbr_plan) are
 * unchanged, and the table is read only through sel.  horizon_selection = 1 selects the static columns by
 * srb_knn_obs_horizon_kernel (with srb12_ctx_set_scenes its scene form) over this context's N and Ts, the agent's own
 * prediction constant velocity from (x0[0], x0[6], x0[1], x0[7]); the neighbour columns by the snapshot or by plans.
 * `plans` may be NULL in all three: the call then extends srb12_solve_batch[_device] / srb12_rollout_device, else
 * srb12_solve_batch_plans[_device] / srb12_rollout_plans_device.  With mv == NULL or mv->obs_vel == NULL each is
 * that entry point, output bits included; a table of zeros gives the same bits as no table.
 *
 * srb12_obstacles_advance_device: srb_obstacles_advance_device with this context's Ts,
 *     obstacles[i][d] = obstacles[i][d] + obs_vel[i][d] * (Ts * 4.0).
 *
 * srb12_rollout_moving_device: per cycle c it enqueues the agents' advance; for c > c_first the obstacle advance; the
 * metrics (unchanged: agents and obstacles are read at matching times); select + solve with the table; with plans,
 * after the solve, the shift as srb12_rollout_plans_device does it.  Plain launches, no host synchronisation; scenes
 * are honoured; a sharded batch is refused as by srb12_rollout_device.
 *
 * SRB_ERR_ARG, by name and before anything is launched: a wrong srb_moving.struct_size; obs_vel with
 * batch.obstacles_version != 0; horizon_selection other than 0 or 1, or set without obs_vel; a rollout with obs_vel
 * whose mv->obstacles is missing or is not batch.obstacles.  host_mv holds host pointers, mv device pointers.
 */
int srb12_solve_batch_moving(srb12_ctx *ctx, int n_agents, const srb12_batch *host_io, const srb12_plans *host_plans,
                             const srb_moving *host_mv);
int srb12_solve_batch_moving_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_plans *plans,
                                    const srb_moving *mv, void *stream);
int srb12_obstacles_advance_device(srb12_ctx *ctx, int n_obs, double *obstacles, const double *obs_vel, void *stream);
int srb12_rollout_moving_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                                const srb12_plans *plans, const srb_moving *mv, int cycles, void *stream);

/*
 * Obstacle sizes in the SRB-12 mode (DESIGN.md 3 "Obstacle sizes", 10.9): srb_sizes (above), its members with the
 * meaning they have in the LIP mode.  Each entry point takes what the srb12_*_moving entry point it extends takes
 * (`plans` and `mv` may be NULL, as there) plus the srb_sizes.  What differs from the LIP block:
 *   obs_eps     the level of static column j < K_obs of the NLP stage is obs_eps[sel[j]], gathered by the
 *               srb12_kernel_mv_* instances, which a level table selects even without obs_vel; a column without a row
 *               keeps eps_obs, the neighbour columns (constant velocity or nbr_plan) keep eps_nbr.
 *   obs_radius  the metrics are those of srb_sim_metrics_sized_device on the srb12_sim.com rows.
 *   clearance_selection = 1  srb_knn_obs_clear_kernel (with srb12_ctx_set_scenes its scene form) on the agent's CoM
 *               row (x0[0], x0[6], x0[1], x0[7]); with mv->horizon_selection = 1 the key's distance is the horizon's
 *               minimum over this context's N and Ts.  The neighbour columns by the snapshot or by plans, as without.
 * There is no srb12 select entry point: the solve runs the selection itself.  With sz == NULL, or every member NULL / 0,
 * each call is the srb12_*_moving entry point it extends (srb12_sim_metrics_sized_device: srb12_sim_metrics_device),
 * output bits included.  SRB_ERR_ARG, by name and before anything is launched: the refusals of srb_sizes (LIP block),
 * which need no context, and everything the extended entry point refuses.  srb12_rollout_sized_device: the sequence of
 * srb12_rollout_moving_device per cycle with the sized metrics, selection and solve; the tables do not change over a
 * rollout.  host_sz holds host pointers, sz device pointers.
 */
int srb12_solve_batch_sized(srb12_ctx *ctx, int n_agents, const srb12_batch *host_io, const srb12_plans *host_plans,
                            const srb_moving *host_mv, const srb_sizes *host_sz);
int srb12_solve_batch_sized_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_plans *plans,
                                   const srb_moving *mv, const srb_sizes *sz, void *stream);
int srb12_sim_metrics_sized_device(srb12_ctx *ctx, int n_agents, const srb12_sim *sim, const srb_sizes *sz, int cycle,
                                   void *stream);
int srb12_rollout_sized_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                               const srb12_plans *plans, const srb_moving *mv, const srb_sizes *sz, int cycles,
                               void *stream);

/*
 * Agent sizes in the SRB-12 mode (DESIGN.md 3 "Agent sizes", 10.11): srb_agent_sizes (above), its members with the
 * meaning they have in the LIP mode.  Each entry point takes what the srb12_*_sized entry point it extends takes
 * (`plans`, `mv` and `sz` may be NULL, as there) plus the srb_agent_sizes.  Every table has n_all rows in the row order
 * of nbr_state (scene-major with scenes); global agent g = agent_offset + a owns row g.  What differs from the LIP block:
 *   agent_rad   the level of neighbour column j (K_obs <= j < K, sel[j] >= 0) of the NLP stage is
 *               (agent_rad[g] + agent_rad[sel[j]])^2, set by the srb12_kernel_mv_* instances, which any of the four
 *               tables selects; a -1 column keeps eps_nbr.  The column's positions are the snapshot's or nbr_plan's,
 *               as without.
 *   agent_pad   the level of static column j < K_obs becomes (sqrt(e_j) + agent_pad[g])^2, e_j the level after the
 *               obs_eps gather (eps_obs, or obs_eps[sel[j]]); a -1 column is included.
 *   agent_body, collide_cycle  the metrics are those of srb_sim_metrics_agents_device on the srb12_sim.com rows.
 *   clearance_selection = 1  srb_knn_nbr_clear_kernel (with srb12_ctx_set_scenes its scene form) on the agent's CoM
 *               row (x0[0], x0[6], x0[1], x0[7]); with plans->plan_selection = 1 and a plan table the key's distance is
 *               the horizon's minimum.  The static columns as the _sized call selects them.
 * There is no srb12 select entry point: the solve runs the selection itself.  With ag == NULL, or every member NULL / 0,
 * each call is the srb12_*_sized entry point it extends, output bits included.  SRB_ERR_ARG, by name and before
 * anything is launched: the refusals of srb_agent_sizes (LIP block), which need no context -- "has a neighbour table"
 * is the srb12_batch's nbr_state and n_all > 0, for the metrics the srb12_sim's --; with agent_rad or agent_pad,
 * agent_offset < 0 or agent_offset + n_agents > n_all (the kernel reads row agent_offset + a of both unchecked); and
 * everything the extended entry point refuses.  The QP-only solve ignores the tables.  srb12_rollout_agents_device:
 * the sequence of srb12_rollout_sized_device per cycle with the agents metrics, selection and solve; it refuses a
 * shard, as srb12_rollout_device does; the tables do not change over a rollout.  host_ag holds host pointers
 * (agent_rad and agent_pad are staged, n_all rows each; agent_body and collide_cycle are not read by a solve), ag
 * device pointers.
 */
int srb12_solve_batch_agents(srb12_ctx *ctx, int n_agents, const srb12_batch *host_io, const srb12_plans *host_plans,
                             const srb_moving *host_mv, const srb_sizes *host_sz, const srb_agent_sizes *host_ag);
int srb12_solve_batch_agents_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_plans *plans,
                                    const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, void *stream);
int srb12_sim_metrics_agents_device(srb12_ctx *ctx, int n_agents, const srb12_sim *sim, const srb_sizes *sz,
                                    const srb_agent_sizes *ag, int cycle, void *stream);
int srb12_rollout_agents_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                                const srb12_plans *plans, const srb_moving *mv, const srb_sizes *sz,
                                const srb_agent_sizes *ag, int cycles, void *stream);

/*
 * Disturbed plant of the SRB-12 mode (DESIGN.md 3 "Disturbed plant", 9, 10.13): srb_plant for the 12-state body -- kicks
 * on velocity, position and angular velocity, pushes, and a body whose mass and inertia are not the model's, or whose
 * dynamics are evaluated where it is and not where the model linearised.  SRB_ABI_VERSION and every existing struct
 * stay; the struct travels through entry points of its own, which extend srb12_sim_advance_device and
 * srb12_rollout_agents_device (plans, mv, sz, ag may be NULL) and otherwise behave as those.  Every table has n_all
 * rows in the row order of nbr_state (scene-major with scenes); global agent g = agent_offset + a owns row g
 * (srb12_sim's agent_offset / n_all; n_all == 0 reads as n_agents rows).  All pointers are device pointers.  All
 * arithmetic is fp64, uncontracted, with one stated grouping (csrc/srb12_plant.hip; tests/plant12_oracle.py restates
 * it: bit for bit, except what passes through the roll's cos / sin).
 *
 * The plant acts in the advance of a cycle c > c_first (at c_first the state is the caller's, as ever) and replaces
 * "state = x[a][36..47]" by state = z + d, one rounded add per component (srb12_plant_state_kernel, one thread per
 * agent; then srb12_sim_advance_plant_kernel, the advance on that state):
 *   z, the base state
 *     plant_mass, plant_inertia NULL and at_state 0    x[a][36..47], the nominal prediction.
 *     otherwise             a four-step roll from the state that started cycle c - 1 -- read from `state` before it is
 *                           overwritten, together with the xref, foot and contact of cycle c - 1, which the advance
 *                           then overwrites, so this advance is NOT idempotent: call it once per cycle.  Step
 *                           k = 0 .. 3 applies the input the model applied, U_k = x[a][12N + 12k .. 12N + 12k + 11],
 *                           with the footholds and contact flags of grid k, by orc12_dynamics' forward-Euler map:
 *                             p' = p + Ts v;  Theta' = Theta + Ts Rz(psi)^T omega;
 *                             v' = v + (Ts / m_g) sum_on f_l + (0, 0, -Ts grav);
 *                             omega' = omega + sum_on Ts I_w^-1 [r_l]x f_l,
 *                           I_w = Rz (s_g I_b) Rz^T, r_l = foot_kl - p^; a leg with contact 0 contributes nothing.
 *                           m_g = plant_mass[g] (NULL: the context's mass), s_g = plant_inertia[g] (NULL: 1).  The
 *                           linearisation point (psi, p^) is, with at_state 0, the model's -- the start state for
 *                           k = 0, sim.xref[a][k - 1] of cycle c - 1 for k >= 1 -- and with at_state 1 the plant's
 *                           own current state z at every step.  No gyroscopic term, no sub-stepping.
 *   d, the disturbance in state order (p, Theta, v, omega), from +0.0
 *     kick_v, kick_p [n_all]  srb_plant's planar kicks, word for word: Philox4x32-10, key ((uint32)seed,
 *                           (uint32)(seed >> 32)), counter ((uint32)c, (uint32)g, 0, 0) gives w0 .. w3,
 *                           u_i = ((double)(int32_t)w_i + 0.5) * 2^-31; dv_x += kick_v[g] u0, dv_y += kick_v[g] u1,
 *                           dp_x += kick_p[g] u2, dp_y += kick_p[g] u3.  A LIP rollout and an SRB-12 rollout with one
 *                           seed therefore get the same planar kicks.
 *     kick_w [n_all]        counter (c, g, 1, 0): domega_i += kick_w[g] u_i for i = 0 .. 2 (w3 is unused).
 *     pushes                every entry p, in table order, with push_cycle[p] == c and push_agent[p] == g adds
 *                           push_dv[p][0..2] to dv and push_dv[p][3..5] to domega, after the kicks.  An entry whose
 *                           cycle is <= c_first, or is never reached, does not fire.
 *                           Each of these steps is one rounded multiply and / or one rounded add.
 *   dist_log [T][A][12]     out, optional: row c - c_first - 1 gets d (columns 2 .. 5 are always 0).
 * Everything an advance derives from the state follows from the new state; the plan shift and the logs of the previous
 * solve are untouched, so a neighbour's shifted plan is stale by the disturbance, as it would be on a robot.
 *
 * With plant == NULL, or every table NULL, at_state 0 and n_push 0, each entry point is the one it extends
 * (srb12_sim_advance_device, srb12_rollout_agents_device): it launches the existing kernels and gives their bits
 * (dist_log is then not written).  SRB_ERR_ARG, by name, before anything is launched: a wrong struct_size; n_push
 * outside 0 .. 4096; n_push > 0 with push_cycle, push_agent or push_dv missing; at_state other than 0 or 1; a roll
 * with srb12_sim.x, xref, foot or contact missing (the advance; the rollout wires them itself).  With a context:
 * agent_offset + n_agents beyond n_all.  The contents of the tables are NOT checked.  srb12_rollout_plant_device
 * refuses a shard, as srb12_rollout_device does; the tables do not change over a rollout.
 */
typedef struct srb12_plant {
    int struct_size;                 /* sizeof(srb12_plant) (ABI check) */
    unsigned long long seed;         /* the Philox key, as srb_plant */
    const double *kick_v;            /* [n_all] m/s   bound on (v_x, v_y) per cycle, or NULL */
    const double *kick_p;            /* [n_all] m     bound on (p_x, p_y) per cycle, or NULL */
    const double *kick_w;            /* [n_all] rad/s bound on omega (3) per cycle, or NULL */
    const double *plant_mass;        /* [n_all] kg, or NULL: the model's mass */
    const double *plant_inertia;     /* [n_all] factor on the model's I_b, or NULL: 1 */
    int at_state;                    /* 1: the plant's dynamics are evaluated at its own state */
    int n_push;                      /* 0 .. 4096 */
    const int *push_cycle, *push_agent;   /* [n_push]; agent = global row */
    const double *push_dv;           /* [n_push][6]: dv (3) m/s, domega (3) rad/s */
    double *dist_log;                /* [T][A][12] out, optional: d in state order */
} srb12_plant;
int srb12_sim_advance_plant_device(srb12_ctx *ctx, int n_agents, const srb12_sim *sim, const srb12_plant *plant,
                                   int cycle, void *stream);
int srb12_rollout_plant_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                               const srb12_plans *plans, const srb_moving *mv, const srb_sizes *sz,
                               const srb_agent_sizes *ag, const srb12_plant *plant, int cycles, void *stream);

/*
 * Degraded neighbour link of the SRB-12 mode (DESIGN.md 3 "Degraded link", 9, 10.15): srb_link, reused as it is, as
 * srb_moving, srb_sizes and srb_agent_sizes are.  SRB_ABI_VERSION and every existing struct stay.  The SRB-12 snapshot
 * row last_state [A][4] and the plan tables [A][N][2] have the LIP layouts and one cycle is 4 grids in both modes, so
 * the update is srb_link_update_kernel unchanged (N and Ts are this context's) and gives the bits of
 * tests/link_oracle.py.  The solve and its selection read the PERCEIVED tables; metrics, traj and every log keep the
 * truth.
 *
 * Unlike the LIP mode (whose refusal of SRB_OPT_PLAN_SELECTION = 1 under a link stays as it is), this mode has the
 * horizon-aware selection under a link: srb_knn_plan_kernel / srb_knn_plan_scene_kernel take an optional table
 * own_plan [n_agents][N][2], indexed by the local agent, and read the agent's own plan points there instead of row
 * agent_offset + a of nbr_plan -- which under a link is a stale, noisy copy of what the agent knows exactly.  The keys
 * of all other rows still come from nbr_state / nbr_plan, and row agent_offset + a stays left out of the scan.
 *
 * srb12_link_update_device: srb_link_update_device on an SRB-12 context, ordered by it.
 * srb12_solve_batch_link_device: srb12_solve_batch_agents_device (plans, mv, sz, ag may be NULL) with own_plan (a device
 * pointer).  own_plan == NULL is that entry point, bit for bit and launch for launch.  SRB_ERR_ARG, by name, before
 * anything is launched: own_plan without plans->plan_selection = 1; own_plan overlapping plans->plan; own_plan together
 * with srb_agent_sizes.clearance_selection = 1 (that selection reads its own plan from the table: not built).
 * srb12_rollout_link_device extends srb12_rollout_plant_device (which is this call with link == NULL): after the metrics
 * of every cycle the update runs on sim.last_state / plans->plan_table, the solve reads link->seen_state as its
 * nbr_state and, from the second cycle with plans, link->seen_plan as its nbr_plan, and with plans->plan_selection
 * plans->plan_table (the truth) as its own_plan; the shift after the solve writes the truth plan_table as ever.  Plain
 * launches, no host synchronisation; scenes are honoured (rows of a perceived table are global rows).
 *
 * With link == NULL or all four tables NULL nothing new is launched and every output has its old bits.  The refusals
 * are srb_rollout_link_device's, by name and before anything is launched -- a wrong struct_size; max_delay outside
 * 0 .. 16; extrapolate not 0 / 1; a link that is on without ring_state, held_state, held_cycle or seen_state; with
 * plans, without ring_plan, held_plan or seen_plan; seen_state overlapping last_state; seen_plan overlapping plan_table
 * or plans->plan; a shard in the driver -- except the plan selection's, which is built here.
 */
int srb12_link_update_device(srb12_ctx *ctx, int n_all, const srb_link *link, const double *last_state,
                             const double *plan_table, int cycle, int c_first, void *stream);
int srb12_solve_batch_link_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_plans *plans,
                                  const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                                  const double *own_plan, void *stream);
int srb12_rollout_link_device(srb12_ctx *ctx, int n_agents, const srb12_batch *dev_io, const srb12_sim *sim,
                              const srb12_plans *plans, const srb_moving *mv, const srb_sizes *sz,
                              const srb_agent_sizes *ag, const srb12_plant *plant, const srb_link *link, int cycles,
                              void *stream);

const char *srb_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
