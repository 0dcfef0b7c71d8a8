// Host side of the SRB-12 extension-mode entry points of include/srbnmpc.h (srb12_*).
//
// The context owns device staging for the host-buffer entry point, a LIP-mode context whose
// selection machinery (srb_knn_kernel and its grids, srb_capi.cpp) it reuses for the obstacle /
// neighbour rows, and events around the two launches.  One 64-lane workgroup per agent runs
// srb12_kernel_<TL>_<TO>_<NC>_<K1> (srb12_kernels.hip): row-slot trips per lane, (N, K) compiled in or 0.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_host.h"

#define SRB12_DBG_LEN (2 * 64 * 8 + 16 + 128)   // trace, stamp sums, state checks (srb12_kernels.hip)
#define SRB12_SIM_NDOMAIN 4                     // grids a cycle (srb12_sim.hip): the shift of the plans between cycles

typedef void (*srb12_fn)(Srb12KParams, int, const double *, const double *, const double *, const int *,
                         const double *, const double *, const int *, double *, double *, double *, int *, int *,
                         const double *, double *);
// the instance's table kernel (srb12_kernel_mv_*): five more arguments, the velocity table of srb_moving, the level
// table of srb_sizes, the radius and pad tables of srb_agent_sizes (each may be null) and the agent_offset of the agent
// tables' own row
typedef void (*srb12_mv_fn)(Srb12KParams, int, const double *, const double *, const double *, const int *,
                            const double *, const double *, const int *, double *, double *, double *, int *, int *,
                            const double *, double *, const double *, const double *, const double *, const double *,
                            int);
// (each kernel's name stands beside its pointer, both from the one pasted token: srb12_ctx_last_kernel reports it)
struct srb12_inst { int tl, to, nc, k1; srb12_fn fn; const char *fn_name; srb12_mv_fn fn_mv; const char *fn_mv_name; };
#define ENTRY12_FN_(f) f, #f
#define ENTRY12(TL, TO, NC, K1) {TL, TO, NC, K1, ENTRY12_FN_(srb12_kernel_##TL##_##TO##_##NC##_##K1), ENTRY12_FN_(srb12_kernel_mv_##TL##_##TO##_##NC##_##K1)},
static const srb12_inst g_inst12[] = {SRB12_INSTANCES(ENTRY12)};
#undef ENTRY12
#undef ENTRY12_FN_

struct srb12_ctx {
    srb12_params p;
    int max_agents, device;
    srb_ctx *sel_ctx;              // LIP-mode context: selection kernels, grids, default sel buffer
    hipStream_t stream;
    hipEvent_t ev[3];
    SrbCallOrder order;            // submission-order chaining of the calls on this context
    bool timed;
    int timing;                    // srb12_ctx_set_timing (default 1)
    double *pos;                   // [max_agents][4] CoM rows for the selection
    int *sel;                      // [max_agents][2 SRB_KNN_MAX]
    double *x0, *xref, *foot, *obstacles, *nbr, *x_qp, *x, *obj;
    int *contact, *status, *iters;
    size_t cap_obs, cap_nbr;
    double *nbr_plan, *plan;       // staging of srb12_solve_batch_plans: the table [cap_plan bytes], the plans [max_agents][N][2]
    size_t cap_plan;
    double *obs_vel;               // staged obstacle velocities [cap_vel bytes] (srb12_solve_batch_moving)
    size_t cap_vel;
    double *obs_eps;               // staged obstacle levels [cap_eps bytes] (srb12_solve_batch_sized)
    size_t cap_eps;
    double *agent_rad, *agent_pad; // staged agent tables [cap_rad / cap_pad bytes] (srb12_solve_batch_agents)
    size_t cap_rad, cap_pad;
    int dbg_agent;                 // diagnostics: srb12_debug_trace
    double *dbg;
    const char *last_solve_name;   // the solve kernel the last launch ran (srb12_ctx_last_kernel)
};

extern "C" void srb12_params_default(srb12_params *p, int N)
{
    std::memset(p, 0, sizeof(*p));
    p->N = N; p->K_obs = 3; p->K_nbr = 0;
    p->Ts = 43 * 0.001;                     // the LIP grid (MPC_dist.cpp:104): the same neighbour prediction
    p->mass = 12.4530;                      // fast_MPC.cpp:40
    const double Ib[9] = {0.01683993, 8.3902e-5, 0.000597679, 8.3902e-5, 0.056579028, 2.5134e-5,
                          0.000597679, 2.5134e-5, 0.064713601};      // fast_MPC.cpp:41-43
    std::memcpy(p->Ib, Ib, sizeof Ib);
    p->grav = 9.81; p->mu = 0.7; p->fmax = 150.0;                   // mu_MPC (Parameters.cpp:32)
    for (int i = 0; i < 12; i++) { p->q[i] = 1e3; p->qN[i] = 1e3; }  // Parameters.cpp:34-45
    for (int i = 0; i < 3; i++) p->r[i] = 1e-2;                      // Parameters.cpp:50-52
    p->Sw = 3000.0;
    p->eps_obs = (double)1.9f; p->eps_nbr = (double)2.2f;
    p->tol = 1e-6; p->qp_maxit = 25; p->nlp_maxit = 50; p->use_nlp = 1;
    p->z0 = 100.0;
    p->tol_final = 1e-8;
    p->polish = 1;
    p->tol_qp = 1e-3;
}

extern "C" int srb12_nv(const srb12_params *p) { return 24 * p->N + 1; }

// the first instance with enough leg-slot and obstacle-slot trips (the list is ordered by cost) for
// horizon N and K rows per grid -- the rows the launch actually selects (clamp_rows: a compiled-in K
// must equal them, the kernel reads sel at that stride and carves its LDS for them)
static const srb12_inst *pick12(int N, int K)
{
    const int tl = srb12_leg_trips(N), to = srb12_obs_trips(N, K);
    for (const srb12_inst &in : g_inst12)      // the (N, K) compiled in
        if (in.nc == N && in.k1 == K + 1 && in.tl >= tl && in.to >= to) return &in;
    for (const srb12_inst &in : g_inst12)      // run-time (N, K)
        if (in.nc == 0 && in.tl >= tl && in.to >= to) return &in;
    return nullptr;
}

static int validate12(const srb12_params *p)
{
    if (!p) return srb_internal_fail(SRB_ERR_ARG, "null params");
    if (p->N < 1 || p->N > SRB12_MAX_N) return srb_internal_fail(SRB_ERR_SIZE, "SRB-12 mode: need 1 <= N <= 24");
    if (p->K_obs < 0 || p->K_nbr < 0 || p->K_obs > SRB_KNN_MAX || p->K_nbr > SRB_KNN_MAX)
        return srb_internal_fail(SRB_ERR_ARG, "K_obs, K_nbr out of range (each <= 16)");
    if (!(p->mass > 0) || !(p->Ts > 0) || !(p->tol > 0) || !(p->tol_final > 0) || !(p->mu >= 0) || !(p->fmax > 0) ||
        !(p->Sw > 0) || !(p->tol_qp >= 0))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_params out of range (mass, Ts, tol, tol_final, fmax, Sw > 0, tol_qp >= 0)");
    for (int i = 0; i < 12; i++)
        if (!(p->q[i] >= 0) || !(p->qN[i] >= 0)) return srb_internal_fail(SRB_ERR_ARG, "state weights must be >= 0");
    for (int i = 0; i < 3; i++)
        if (!(p->r[i] > 0)) return srb_internal_fail(SRB_ERR_ARG, "force weights must be > 0");
    if (!pick12(p->N, p->K_obs + p->K_nbr)) return srb_internal_fail(SRB_ERR_SIZE, "no SRB-12 kernel instance covers the row slots");
    if ((size_t)srb12_lds_doubles(p->N, p->K_obs + p->K_nbr) * sizeof(double) > 160 * 1024)
        return srb_internal_fail(SRB_ERR_SIZE, "per-agent LDS exceeds 160 KiB");
    return SRB_OK;
}

// the parameter checks of srb12_ctx_create alone (no device needed)
extern "C" int srb12_check_params(const srb12_params *p) { return validate12(p); }

// the instance table and the pick, host only (no HIP call: usable without a device)
extern "C" int srb12_kernel_table(int i, int dims[4], const char **name)
{
    if (i < 0 || i >= (int)(sizeof g_inst12 / sizeof g_inst12[0])) return srb_internal_fail(SRB_ERR_ARG, "srb12_kernel_table: index past the end");
    const srb12_inst &in = g_inst12[i];
    if (dims) { dims[0] = in.tl; dims[1] = in.to; dims[2] = in.nc; dims[3] = in.k1; }
    if (name) *name = in.fn_name;
    return SRB_OK;
}

extern "C" int srb12_pick_kernel(int N, int K, int dims[4])
{
    if (!dims || N < 1 || K < 0) return srb_internal_fail(SRB_ERR_ARG, "srb12_pick_kernel: bad argument");
    const srb12_inst *in = pick12(N, K);
    if (!in) return srb_internal_fail(SRB_ERR_SIZE, "no SRB-12 kernel instance covers the row slots");
    dims[0] = in->tl; dims[1] = in->to; dims[2] = in->nc; dims[3] = in->k1;
    return SRB_OK;
}

extern "C" int srb12_ctx_last_kernel(srb12_ctx *c, const char **solve)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    if (solve) *solve = c->last_solve_name ? c->last_solve_name : "";
    return SRB_OK;
}

extern "C" int srb12_lds_bytes(const srb12_params *p)
{
    return p ? srb12_lds_doubles(p->N, p->K_obs + p->K_nbr) * (int)sizeof(double) : -1;
}

static Srb12KParams make_k12(const srb12_params *p, int K_obs, int K_nbr)
{
    Srb12KParams k;
    std::memset(&k, 0, sizeof k);
    k.N = p->N; k.K_obs = K_obs; k.K_nbr = K_nbr; k.use_nlp = p->use_nlp ? 1 : 0;
    k.qp_maxit = p->qp_maxit; k.nlp_maxit = p->nlp_maxit;
    k.Ts = p->Ts; k.mass = p->mass; k.grav = p->grav; k.mus = p->mu / std::sqrt(2.0); k.fmax = p->fmax;
    k.Sw = p->Sw; k.eps_obs = p->eps_obs; k.eps_nbr = p->eps_nbr; k.tol = p->tol; k.z0 = p->z0; k.tol_final = p->tol_final; k.polish = p->polish ? 1 : 0;
    k.tol_qp = p->tol_qp;
    std::memcpy(k.Ib, p->Ib, sizeof k.Ib);
    std::memcpy(k.q, p->q, sizeof k.q); std::memcpy(k.qN, p->qN, sizeof k.qN); std::memcpy(k.r, p->r, sizeof k.r);
    return k;
}

extern "C" int srb12_ctx_create(const srb12_params *p, int max_agents, int device, srb12_ctx **out)
{
    if (!out || max_agents <= 0) return srb_internal_fail(SRB_ERR_ARG, "bad arguments");
    int rc = validate12(p);
    if (rc) return rc;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return srb_internal_fail(SRB_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    srb_params sp;
    srb_params_default(&sp, 2, 2);
    sp.K_obs = p->K_obs; sp.K_nbr = p->K_nbr;
    srb_ctx *sc = nullptr;
    if ((rc = srb_ctx_create(&sp, max_agents, device, &sc))) return rc;
    srb12_ctx *c = new srb12_ctx();
    std::memset(c, 0, sizeof *c);
    // a failure after this point unwinds through srb12_ctx_destroy (it null-checks every buffer and
    // destroys the selection context); *out stays untouched
    c->p = *p; c->max_agents = max_agents; c->device = device; c->sel_ctx = sc;
    const size_t A = (size_t)max_agents, N = (size_t)p->N, nv = 24 * N + 1;
#define CREATE_CHK(expr) HIPCHK_UNWIND_(expr, #expr, srb12_ctx_destroy(c))
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) CREATE_CHK(hipEventCreate(&c->ev[i]));
    CREATE_CHK(hipEventCreateWithFlags(&c->order.done, hipEventDisableTiming));
    CREATE_CHK(hipMalloc(&c->pos, A * 4 * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->sel, A * 2 * SRB_KNN_MAX * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->x0, A * 12 * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->xref, A * 12 * N * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->foot, A * 12 * N * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->contact, A * 4 * N * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->x_qp, A * nv * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->x, A * nv * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->obj, A * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->status, A * 2 * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->iters, A * 2 * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->dbg, SRB12_DBG_LEN * sizeof(double)));
#undef CREATE_CHK
    c->dbg_agent = -1; c->timing = 1;
    *out = c;
    return SRB_OK;
}

extern "C" int srb12_ctx_destroy(srb12_ctx *c)
{
    if (!c) return SRB_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)c->order.wait_idle();
    void *bufs[] = {c->dbg, c->pos, c->sel, c->x0, c->xref, c->foot, c->contact, c->obstacles, c->nbr, c->x_qp, c->x, c->obj,
                    c->status, c->iters, c->nbr_plan, c->plan, c->obs_vel, c->obs_eps, c->agent_rad, c->agent_pad};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    for (int i = 0; i < 3; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->order.done) (void)hipEventDestroy(c->order.done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    srb_ctx_destroy(c->sel_ctx);
    delete c;
    return SRB_OK;
}

// "up to K nearest": the rows selected per agent, clamped to what the tables hold (batch-uniform, as
// the LIP mode; with scenes to the agent's scene: scene_obs rows, scene_agents - 1 others) and 0 without
// the NLP stage -- the launch and the host copy-back of sel use this one rule
static void clamp_rows(const srb12_ctx *c, const srb12_batch *d, int *Ko, int *Kn)
{
    int ko = c->p.K_obs, kn = c->p.K_nbr;
    srb_internal_clamp_K(c->sel_ctx, d->n_obs, d->nbr_state != nullptr, d->n_all, &ko, &kn);
    if (!c->p.use_nlp) ko = kn = 0;
    *Ko = ko; *Kn = kn;
}

// the per-call refusals of the scene partition (srb12_ctx_set_scenes), the LIP mode's with its messages
static int check_scenes12(const srb12_ctx *c, int n_agents, const srb12_batch *d)
{
    return srb_internal_check_scenes(c->sel_ctx, n_agents, d->n_obs, d->nbr_state != nullptr, d->n_all, d->agent_offset);
}

// The argument errors of srb12_plans that need no context, in a fixed order (struct_size first); `rollout`: the
// driver's rules (plan and plan_table required, nbr_state is the rollout's own snapshot, and plan_selection waits
// for the first cycle that has a table)
static int check_plans12(const srb12_batch *b, const srb12_plans *pl, bool rollout)
{
    if (int rc = srb_check_struct(pl, "srb12_plans")) return rc;
    if (!b || !pl) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (pl->plan_selection != 0 && pl->plan_selection != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_plans.plan_selection: 0 (snapshot) or 1 (closest predicted approach)");
    if (rollout && (!pl->plan || !pl->plan_table))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_rollout_plans_device needs srb12_plans.plan and plan_table");
    if (!rollout && pl->nbr_plan && !b->nbr_state)
        return srb_internal_fail(SRB_ERR_ARG, "nbr_plan needs nbr_state (the selection's snapshot)");
    if (!rollout && pl->plan_selection && !pl->nbr_plan)
        return srb_internal_fail(SRB_ERR_ARG, "plan_selection = 1 needs nbr_plan (the horizon-aware selection reads the plan table)");
    if (pl->plan && (const double *)pl->plan == pl->nbr_plan)
        return srb_internal_fail(SRB_ERR_ARG, "plan overlaps the nbr_plan table (workgroups read the table while others write "
                                              "their plans: use two buffers)");
    if (pl->plan && pl->plan == pl->plan_table)
        return srb_internal_fail(SRB_ERR_ARG, "plan overlaps plan_table (the shift reads one and writes the other: use two buffers)");
    return SRB_OK;
}

// the checks of srb_moving, srb_sizes and srb_agent_sizes that need no context (srb_host.h), with this mode's names in
// the messages
static int check_tables12(const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, const srb12_batch *b,
                          bool rollout)
{
    return srb_check_tables(mv, sz, ag, b, rollout, "srb12_rollout_moving_device", "srb12_batch");
}

// pl: the plan members of this launch (NULL: none, the launch of srb12_solve_batch[_device] as ever); t: the tables of
// srb_moving, srb_sizes and srb_agent_sizes (SrbTables{}: none, every launch as without them); own_plan
// [n_agents][N][2]: with pl->plan_selection the agent's own plan of the horizon-aware selection (null: row
// agent_offset + a of pl->nbr_plan, the launch as before)
static int launch12(srb12_ctx *c, int n_agents, const srb12_batch *d, hipStream_t s, const srb12_plans *pl,
                    const SrbTables &t, const double *own_plan = nullptr)
{
    if (n_agents < 0 || n_agents > c->max_agents) return srb_internal_fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    const srb12_params *p = &c->p;
    if (!d->x0 || !d->xref || !d->foot || !d->contact || !d->x || !d->obj || !d->status || !d->iters)
        return srb_internal_fail(SRB_ERR_ARG, "missing buffer");
    if (p->use_nlp && p->K_obs > 0 && (d->n_obs < 0 || (d->n_obs > 0 && !d->obstacles)))
        return srb_internal_fail(SRB_ERR_ARG, "obstacles missing");
    if (p->use_nlp && p->K_nbr > 0 && d->nbr_state && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return srb_internal_fail(SRB_ERR_ARG, "agent_offset out of range of the neighbour table");
    if (pl && pl->nbr_plan && p->K_nbr > 0 && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return srb_internal_fail(SRB_ERR_ARG, "nbr_plan: agent_offset + n_agents exceeds n_all (the plan table's rows)");
    // (the kernel reads row agent_offset + agent of the agent tables unchecked)
    if (p->use_nlp && (t.agent_rad || t.agent_pad) && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes: agent_offset + n_agents exceeds n_all (the agent tables' rows)");
    if (pl && pl->plan) {
        const size_t rows = (size_t)n_agents * 2 * p->N;
        if (srb_overlap(pl->plan, rows, pl->nbr_plan, (size_t)(d->n_all > 0 ? d->n_all : 0) * 2 * p->N) ||
            srb_overlap(pl->plan, rows, pl->plan_table, rows))
            return srb_internal_fail(SRB_ERR_ARG, "plan overlaps the nbr_plan table or plan_table (use two buffers)");
        if (srb_overlap(pl->plan, rows, own_plan, rows))
            return srb_internal_fail(SRB_ERR_ARG, "own_plan overlaps srb12_plans.plan (the selection reads one while the solve "
                                                  "writes the other: use two buffers)");
    }
    if (int rc = check_scenes12(c, n_agents, d)) return rc;
    int Ko = 0, Kn = 0;
    clamp_rows(c, d, &Ko, &Kn);
    // (the table is read by the NLP stage's neighbour rows only: without them it is never touched)
    const double *nbr_plan = (pl && p->use_nlp && Kn > 0 && d->nbr_state) ? pl->nbr_plan : nullptr;
    // (the velocities, levels and pads are read by the NLP stage's static rows only, through sel; the radii by its
    // neighbour columns only, through sel and at the agent's own row; the QP-only solve reads none)
    const SrbTables g = t.gated(p->use_nlp && Ko > 0, p->use_nlp && Kn > 0);
    const double *vel = g.obs_vel, *eps = g.obs_eps, *rad = g.agent_rad, *pad = g.agent_pad;
    Srb12KParams k = make_k12(p, Ko, Kn);
    k.dbg_agent = c->dbg_agent; k.dbg = c->dbg;
    const srb12_inst *in = pick12(p->N, Ko + Kn);
    if (!in) return srb_internal_fail(SRB_ERR_SIZE, "no SRB-12 kernel instance covers the row slots");
    const size_t lds = (size_t)srb12_lds_doubles(p->N, Ko + Kn) * sizeof(double);
    int *sel = d->sel ? d->sel : c->sel;
    if (c->timing) HIPCHK(hipEventRecord(c->ev[0], s));
    if (Ko + Kn > 0) {
        hipLaunchKernelGGL(srb12_pos_kernel, dim3((n_agents + 255) / 256), dim3(256), 0, s, n_agents, d->x0, c->pos);
        HIPCHK(hipGetLastError());
        SrbSelect q = {};
        q.n_agents = n_agents; q.x0 = c->pos; q.agent_offset = d->agent_offset;
        q.obstacles = d->obstacles; q.n_obs = Ko > 0 ? d->n_obs : 0; q.obstacles_version = d->obstacles_version;
        q.nbr_state = d->nbr_state; q.n_all = Kn > 0 ? d->n_all : 0;
        q.K_obs = Ko; q.K_nbr = Kn; q.sel = sel; q.s = s;
        q.N = p->N; q.Ts = p->Ts;
        q.nbr_plan = pl && pl->plan_selection ? nbr_plan : nullptr;
        q.own_plan = q.nbr_plan ? own_plan : nullptr;
        q.t = g;
        int rc = srb_internal_select(c->sel_ctx, q);
        if (rc) return rc;
        // the selection context's own ordering event: its grid buffers are reallocated only after
        // this launch (grid_reserve waits on it)
        if ((rc = srb_internal_mark_done(c->sel_ctx, s))) return rc;
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev[1], s));
    // with any of the four tables the instance's table kernel (five more arguments); without, the launch as ever
    c->last_solve_name = g.any_solve_table() ? in->fn_mv_name : in->fn_name;
    if (g.any_solve_table())
        hipLaunchKernelGGL(in->fn_mv, dim3(n_agents), dim3(64), lds, s, k, n_agents, d->x0, d->xref, d->foot, d->contact,
                           d->obstacles, d->nbr_state, (const int *)sel, d->x_qp, d->x, d->obj, d->status, d->iters,
                           nbr_plan, pl ? pl->plan : nullptr, vel, eps, rad, pad, d->agent_offset);
    else
        hipLaunchKernelGGL(in->fn, dim3(n_agents), dim3(64), lds, s, k, n_agents, d->x0, d->xref, d->foot, d->contact,
                           d->obstacles, d->nbr_state, (const int *)sel, d->x_qp, d->x, d->obj, d->status, d->iters, nbr_plan,
                           pl ? pl->plan : nullptr);
    HIPCHK(hipGetLastError());
    if (c->timing) HIPCHK(hipEventRecord(c->ev[2], s));
    c->timed = c->timing != 0;
    return SRB_OK;
}

// The argument errors of an own plan that need no context (srb12_solve_batch_link_device; the driver hands over
// plan_table, which check_plans12 keeps apart from plan)
static int check_own_plan12(const double *own_plan, const srb12_plans *pl, const srb_agent_sizes *ag)
{
    if (!own_plan) return SRB_OK;
    if (!pl || pl->plan_selection != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_solve_batch_link_device: own_plan needs srb12_plans.plan_selection = 1 "
                                              "(only the horizon-aware selection reads the agent's own plan)");
    if (own_plan == pl->plan)
        return srb_internal_fail(SRB_ERR_ARG, "own_plan overlaps srb12_plans.plan (the selection reads one while the solve "
                                              "writes the other: use two buffers)");
    if (ag && ag->agent_rad && ag->clearance_selection)
        return srb_internal_fail(SRB_ERR_ARG, "own_plan with srb_agent_sizes.clearance_selection = 1: the clearance selection "
                                              "reads the agent's own plan from its row of the table (not built)");
    return SRB_OK;
}

// pl, mv, sz and ag may be NULL; own_plan NULL: srb12_solve_batch_agents_device itself.  (Every device solve comes
// this way: one path.)
extern "C" int srb12_solve_batch_link_device(srb12_ctx *c, int n_agents, const srb12_batch *d, const srb12_plans *pl,
                                             const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                                             const double *own_plan, void *stream)
{
    if (int rc = srb_check_struct(d, "srb12_batch")) return rc;
    if (int rc0 = check_tables12(mv, sz, ag, d, false)) return rc0;
    if (pl)
        if (int rc = check_plans12(d, pl, false)) return rc;
    if (int rc0 = check_own_plan12(own_plan, pl, ag)) return rc0;
    if (!c || !d) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = c->order.order_after_last(s);
    if (!rc) rc = launch12(c, n_agents, d, s, pl, srb_tables(mv, sz, ag), own_plan);
    if (!rc && n_agents > 0) rc = c->order.mark_done(s);
    return rc;
}

// pl, mv and sz may be NULL, as in srb12_solve_batch_sized_device; ag NULL (or without a table): that entry point itself.
// (The _sized and the _moving entry points are the _agents ones without a table: one path.)
extern "C" int srb12_solve_batch_agents_device(srb12_ctx *c, int n_agents, const srb12_batch *d, const srb12_plans *pl,
                                               const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                                               void *stream)
{
    return srb12_solve_batch_link_device(c, n_agents, d, pl, mv, sz, ag, nullptr, stream);
}

extern "C" int srb12_solve_batch_sized_device(srb12_ctx *c, int n_agents, const srb12_batch *d, const srb12_plans *pl,
                                              const srb_moving *mv, const srb_sizes *sz, void *stream)
{
    return srb12_solve_batch_agents_device(c, n_agents, d, pl, mv, sz, nullptr, stream);
}

extern "C" int srb12_solve_batch_device(srb12_ctx *c, int n_agents, const srb12_batch *d, void *stream)
{
    return srb12_solve_batch_sized_device(c, n_agents, d, nullptr, nullptr, nullptr, stream);
}

// (this entry point needs its struct)
extern "C" int srb12_solve_batch_plans_device(srb12_ctx *c, int n_agents, const srb12_batch *d, const srb12_plans *pl,
                                              void *stream)
{
    if (int rc = srb_check_struct(d, "srb12_batch")) return rc;
    if (!pl) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    return srb12_solve_batch_sized_device(c, n_agents, d, pl, nullptr, nullptr, stream);
}

// pl may be NULL (srb12_solve_batch_device with the table), else srb12_solve_batch_plans_device with it
extern "C" int srb12_solve_batch_moving_device(srb12_ctx *c, int n_agents, const srb12_batch *d, const srb12_plans *pl,
                                               const srb_moving *mv, void *stream)
{
    return srb12_solve_batch_sized_device(c, n_agents, d, pl, mv, nullptr, stream);
}

// hp: the host plan members (NULL: srb12_solve_batch); the table and the plans are staged like the other buffers
static int solve_host12(srb12_ctx *c, int n_agents, const srb12_batch *h, const srb12_plans *hp, bool plans,
                        const srb_moving *hmv = nullptr, const srb_sizes *hsz = nullptr,
                        const srb_agent_sizes *hag = nullptr)
{
    if (int rc = srb_check_struct(h, "srb12_batch")) return rc;
    if (int rc0 = check_tables12(hmv, hsz, hag, h, false)) return rc0;
    if (plans)
        if (int rc = check_plans12(h, hp, false)) return rc;
    if (!c || !h) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (n_agents < 0 || n_agents > c->max_agents) return srb_internal_fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    if (!h->x0 || !h->xref || !h->foot || !h->contact || !h->x || !h->obj || !h->status || !h->iters)
        return srb_internal_fail(SRB_ERR_ARG, "missing buffer");
    if (int rc0 = srb_internal_check_scenes(c->sel_ctx, n_agents, h->obstacles ? h->n_obs : 0, h->n_all > 0 && h->nbr_state,
                                            h->n_all, h->agent_offset))
        return rc0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (int rc0 = c->order.order_after_last(s)) return rc0;
    const size_t A = (size_t)n_agents, N = (size_t)c->p.N, nv = 24 * N + 1;
    HIPCHK(hipMemcpyAsync(c->x0, h->x0, A * 12 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->xref, h->xref, A * 12 * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->foot, h->foot, A * 12 * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->contact, h->contact, A * 4 * N * sizeof(int), hipMemcpyHostToDevice, s));
    srb12_batch d = *h;
    d.x0 = c->x0; d.xref = c->xref; d.foot = c->foot; d.contact = c->contact;
    d.x_qp = c->x_qp; d.x = c->x; d.obj = c->obj; d.status = c->status; d.iters = c->iters;
    d.sel = h->sel ? c->sel : nullptr;
    d.obstacles = nullptr; d.nbr_state = nullptr;
    if (h->n_obs > 0 && h->obstacles) {
        if (int rc = srb_stage_copy(c->order, c->obstacles, c->cap_obs, h->obstacles, (size_t)h->n_obs * 2 * sizeof(double), s))
            return rc;
        d.obstacles = c->obstacles;
    }
    if (h->n_all > 0 && h->nbr_state) {
        if (int rc = srb_stage_copy(c->order, c->nbr, c->cap_nbr, h->nbr_state, (size_t)h->n_all * 4 * sizeof(double), s))
            return rc;
        d.nbr_state = c->nbr;
    }
    d.obstacles_version = 0;               // staging copies: no grid reuse across calls
    srb12_plans dp;
    std::memset(&dp, 0, sizeof dp);
    dp.struct_size = (int)sizeof dp;
    if (hp) {
        dp.plan_selection = hp->plan_selection;
        if (hp->nbr_plan && d.nbr_state) {
            if (c->p.K_nbr > 0 && (h->agent_offset < 0 || h->agent_offset + n_agents > h->n_all))
                return srb_internal_fail(SRB_ERR_ARG, "nbr_plan: agent_offset + n_agents exceeds n_all (the plan table's rows)");
            if (int rc = srb_stage_copy(c->order, c->nbr_plan, c->cap_plan, hp->nbr_plan, (size_t)h->n_all * 2 * N * sizeof(double), s))
                return rc;
            dp.nbr_plan = c->nbr_plan;
        }
        if (hp->plan) {
            if (!c->plan) HIPCHK(hipMalloc(&c->plan, (size_t)c->max_agents * 2 * N * sizeof(double)));
            dp.plan = c->plan;
        }
    }
    // The tables: ht the caller's (host), t their staged copies.  The velocity and the level table are staged like
    // the obstacle rows they belong to (none without them), the agent tables with n_all rows each.  (Only the agent
    // tables ask for the NLP stage here, all four in the LIP mode's solve_host: without it launch12 hands no table to
    // a kernel and selects no rows, so nothing observable depends on the difference.)
    const SrbTables ht = srb_tables(hmv, hsz, hag);
    SrbTables t = {};
    t.obs_horizon = ht.obs_horizon; t.obs_clear = ht.obs_clear; t.nbr_clear = ht.nbr_clear;
    if (ht.obs_vel && d.obstacles) {
        if (int rc = srb_stage_copy(c->order, c->obs_vel, c->cap_vel, ht.obs_vel, (size_t)h->n_obs * 2 * sizeof(double), s))
            return rc;
        t.obs_vel = c->obs_vel;
    }
    if (ht.obs_eps && d.obstacles) {
        if (int rc = srb_stage_copy(c->order, c->obs_eps, c->cap_eps, ht.obs_eps, (size_t)h->n_obs * sizeof(double), s))
            return rc;
        t.obs_eps = c->obs_eps;
    }
    if (c->p.use_nlp && (ht.agent_rad || ht.agent_pad)) {
        if (h->agent_offset < 0 || h->agent_offset + n_agents > h->n_all)    // launch12's refusal, before the copies
            return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes: agent_offset + n_agents exceeds n_all (the agent tables' rows)");
        const size_t bytes = (size_t)h->n_all * sizeof(double);
        if (ht.agent_rad) {
            if (int rc = srb_stage_copy(c->order, c->agent_rad, c->cap_rad, ht.agent_rad, bytes, s)) return rc;
            t.agent_rad = c->agent_rad;
        }
        if (ht.agent_pad) {
            if (int rc = srb_stage_copy(c->order, c->agent_pad, c->cap_pad, ht.agent_pad, bytes, s)) return rc;
            t.agent_pad = c->agent_pad;
        }
    }
    t.normalise();                         // (a table that was not staged takes its flag with it)
    int rc = launch12(c, n_agents, &d, s, hp ? &dp : nullptr, t);
    if (!rc) rc = c->order.mark_done(s);
    if (rc) return rc;
    if (h->x_qp) HIPCHK(hipMemcpyAsync(h->x_qp, c->x_qp, A * nv * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->x, c->x, A * nv * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->obj, c->obj, A * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->status, c->status, A * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->iters, c->iters, A * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (dp.plan) HIPCHK(hipMemcpyAsync(hp->plan, c->plan, A * 2 * N * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h->sel) {
        int Ko = 0, Kn = 0;
        clamp_rows(c, &d, &Ko, &Kn);
        const int Kt = Ko + Kn;
        if (Kt > 0) HIPCHK(hipMemcpyAsync(h->sel, c->sel, A * Kt * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return SRB_OK;
}

extern "C" int srb12_solve_batch(srb12_ctx *c, int n_agents, const srb12_batch *h)
{
    return solve_host12(c, n_agents, h, nullptr, false);
}

extern "C" int srb12_solve_batch_plans(srb12_ctx *c, int n_agents, const srb12_batch *h, const srb12_plans *hp)
{
    return solve_host12(c, n_agents, h, hp, true);
}

// hp may be NULL (srb12_solve_batch with the table), else srb12_solve_batch_plans with it
extern "C" int srb12_solve_batch_moving(srb12_ctx *c, int n_agents, const srb12_batch *h, const srb12_plans *hp,
                                        const srb_moving *hmv)
{
    return srb12_solve_batch_sized(c, n_agents, h, hp, hmv, nullptr);
}

// hp and hmv may be NULL, as in srb12_solve_batch_moving; hsz NULL (or without a table): that entry point itself
extern "C" int srb12_solve_batch_sized(srb12_ctx *c, int n_agents, const srb12_batch *h, const srb12_plans *hp,
                                       const srb_moving *hmv, const srb_sizes *hsz)
{
    return srb12_solve_batch_agents(c, n_agents, h, hp, hmv, hsz, nullptr);
}

// hp, hmv and hsz may be NULL, as in srb12_solve_batch_sized; hag NULL (or without a table): that entry point itself
extern "C" int srb12_solve_batch_agents(srb12_ctx *c, int n_agents, const srb12_batch *h, const srb12_plans *hp,
                                        const srb_moving *hmv, const srb_sizes *hsz, const srb_agent_sizes *hag)
{
    return solve_host12(c, n_agents, h, hp, hp != nullptr, hmv, hsz, hag);
}

extern "C" int srb12_ctx_set_timing(srb12_ctx *c, int on)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    c->timing = on ? 1 : 0;
    return SRB_OK;
}

extern "C" int srb12_last_kernel_ms(srb12_ctx *c, float *select_ms, float *solve_ms)
{
    if (!c || !c->timed) return srb_internal_fail(SRB_ERR_ARG, "no timed launch");
    HIPCHK(hipEventSynchronize(c->ev[2]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    if (select_ms) *select_ms = a;
    if (solve_ms) *solve_ms = b;
    return SRB_OK;
}

// ---- scenes: the partition lives in the selection context, whose kernels and checks serve both modes
extern "C" int srb12_ctx_set_scenes(srb12_ctx *c, int scene_agents, int scene_obs)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    return srb_ctx_set_scenes(c->sel_ctx, scene_agents, scene_obs);
}

extern "C" int srb12_ctx_scenes(srb12_ctx *c, int *scene_agents, int *scene_obs)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    return srb_ctx_scenes(c->sel_ctx, scene_agents, scene_obs);
}

// ---- closed-loop rollout (srb12_sim.hip): the argument checks that need no context come first, in a fixed order
// (struct_size, c_first, goal, x), as check_sim of srb_capi.cpp
static int check_sim12(const srb12_sim *d, int cycle, bool advance)
{
    if (int rc = srb_check_struct(d, "srb12_sim")) return rc;
    if (!d) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (cycle < d->c_first) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim: cycle precedes c_first");
    if (!advance) return SRB_OK;
    if (!d->goal) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim.goal missing");
    if (!d->x && cycle != d->c_first)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_sim.x missing (the previous solve's x: required when cycle != c_first)");
    return SRB_OK;
}

// The argument errors of srb12_plant that need no context, before anything is launched.  d: the advance's srb12_sim,
// whose x, xref, foot and contact a roll reads (null: the rollout, which wires them in and reports what is missing
// itself).
#define SRB12_PLANT_MAX_PUSH 4096
static bool plant12_rolls(const srb12_plant *pl) { return pl->plant_mass || pl->plant_inertia || pl->at_state != 0; }
static int check_plant12(const srb12_plant *pl, const srb12_sim *d)
{
    if (int rc = srb_check_struct(pl, "srb12_plant")) return rc;
    if (!pl) return SRB_OK;
    if (pl->n_push < 0 || pl->n_push > SRB12_PLANT_MAX_PUSH)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_plant.n_push: 0 .. 4096 (every agent scans the whole push table)");
    if (pl->n_push > 0 && (!pl->push_cycle || !pl->push_agent || !pl->push_dv))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_plant.n_push > 0 needs push_cycle, push_agent and push_dv");
    if (pl->at_state != 0 && pl->at_state != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_plant.at_state: 0 the model's linearisation point, 1 the plant's own state");
    if (d && plant12_rolls(pl) && (!d->x || !d->xref || !d->foot || !d->contact))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_plant: plant_mass, plant_inertia and at_state need srb12_sim.x, xref, foot "
                                              "and contact (the plant is driven by the inputs, footholds and contact flags the "
                                              "model applied)");
    return SRB_OK;
}

// the struct disturbs the plant at all (else every entry point is the one it extends; dist_log alone is not written)
static bool plant12_on(const srb12_plant *pl)
{
    return pl && (pl->kick_v || pl->kick_p || pl->kick_w || plant12_rolls(pl) || pl->n_push > 0);
}

// pl: the disturbed plant (null: nominal).  It acts from the second cycle on; at c_first the state is the caller's.
static int launch_advance12(srb12_ctx *c, int n_agents, const srb12_sim *d, int cycle, hipStream_t s,
                            const srb12_plant *pl = nullptr)
{
    const srb12_params *p = &c->p;
    if (p->N < 4) return srb_internal_fail(SRB_ERR_ARG, "the rollout needs N >= 4 (one cycle is one gait domain of 4 grids)");
    if (!d->state || !d->x0 || !d->xref || !d->foot || !d->contact || !d->last_state || !d->com)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_sim: missing buffer (state, x0, xref, foot, contact, last_state, com)");
    if (d->gait != 0 && d->gait != 1) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim.gait: 0 trot, 1 stand");
    const int threads = n_agents * p->N;                  // one per (agent, grid): at most max_agents * 24
    if (pl && cycle != d->c_first) {
        const int n_all = d->n_all > 0 ? d->n_all : n_agents;
        if (d->agent_offset < 0 || d->agent_offset + n_agents > n_all)
            return srb_internal_fail(SRB_ERR_ARG, "srb12_plant: agent_offset + n_agents exceeds n_all (the plant tables' rows)");
        Srb12PlantIb Ib;
        for (int i = 0; i < 9; i++) Ib.v[i] = p->Ib[i];
        // the state z + d, one thread per agent, then the advance on it, one thread per (agent, grid)
        hipLaunchKernelGGL(srb12_plant_state_kernel, dim3((n_agents + 255) / 256), dim3(256), 0, s, n_agents, p->N, p->Ts,
                           p->mass, Ib, p->grav, cycle, d->c_first, d->state, d->x, (const double *)d->xref,
                           (const double *)d->foot, (const int *)d->contact, d->agent_offset,
                           (unsigned)(pl->seed & 0xffffffffull), (unsigned)(pl->seed >> 32), pl->kick_v, pl->kick_p,
                           pl->kick_w, pl->plant_mass, pl->plant_inertia, pl->at_state, plant12_rolls(pl) ? 1 : 0,
                           pl->n_push, pl->push_cycle, pl->push_agent, pl->push_dv, pl->dist_log);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(srb12_sim_advance_plant_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, n_agents, p->N,
                           p->Ts, d->vref, d->hcom, d->yaw_step, d->hold_radius, d->gait, cycle, d->c_first, d->state,
                           d->goal, d->phase, d->x, d->status, d->iters, d->x0, d->xref, d->foot, d->contact,
                           d->last_state, d->com, d->traj, d->status_log, d->iters_log, d->x_log);
        HIPCHK(hipGetLastError());
        return SRB_OK;
    }
    hipLaunchKernelGGL(srb12_sim_advance_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, n_agents, p->N, p->Ts,
                       d->vref, d->hcom, d->yaw_step, d->hold_radius, d->gait, cycle, d->c_first, d->state, d->goal,
                       d->phase, d->x, d->status, d->iters, d->x0, d->xref, d->foot, d->contact, d->last_state, d->com,
                       d->traj, d->status_log, d->iters_log, d->x_log);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// the metrics of the LIP rollout (srb_sim_metrics_kernel, with scenes srb_sim_scene_metrics_kernel) on the com rows;
// t.obs_radius (srb_sizes; null: the centre distances and the 0.5 m fail test, the kernels as ever); t.agent_body and
// t.collide_cycle (srb_agent_sizes; body null: d_agent by centres, the kernels as ever)
static int launch_metrics12(srb12_ctx *c, int n_agents, const srb12_sim *d, int cycle, hipStream_t s, const SrbTables &t)
{
    if (!d->com) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim: missing buffer (com)");
    if (d->n_obs < 0 || d->n_all < 0 || (d->n_obs > 0 && !d->obstacles) || (d->n_all > 0 && !d->nbr_state))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_sim: obstacles / nbr_state missing for n_obs / n_all rows");
    srb_sim m;
    std::memset(&m, 0, sizeof m);
    m.struct_size = (int)sizeof m;
    m.state = d->com; m.c_first = d->c_first;
    m.obstacles = d->obstacles; m.nbr_state = d->nbr_state;
    m.n_obs = d->n_obs; m.n_all = d->n_all; m.agent_offset = d->agent_offset;
    m.d_obs = d->d_obs; m.d_agent = d->d_agent; m.min_d_obs = d->min_d_obs; m.min_d_agent = d->min_d_agent;
    m.fail_cycle = d->fail_cycle; m.distance_to_fail = d->distance_to_fail;
    return srb_internal_sim_metrics(c->sel_ctx, n_agents, &m, cycle, s, t);
}

template <bool advance>
static int sim12_call(srb12_ctx *c, int n_agents, const srb12_sim *d, int cycle, void *stream, const srb_sizes *sz,
                      const srb_agent_sizes *ag, const srb12_plant *pl)
{
    if (int rc = check_sim12(d, cycle, advance)) return rc;
    if (int rc = check_plant12(pl, d)) return rc;
    if (!plant12_on(pl)) pl = nullptr;
    if (int rc = srb_check_sizes(sz)) return rc;
    if (int rc = srb_check_agent_sizes(ag, d->nbr_state && d->n_all > 0)) return rc;
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (n_agents < 0 || n_agents > c->max_agents) return srb_internal_fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] {
        return advance ? launch_advance12(c, n_agents, d, cycle, s, pl)
                       : launch_metrics12(c, n_agents, d, cycle, s, srb_tables(nullptr, sz, ag));
    });
}

extern "C" int srb12_sim_advance_plant_device(srb12_ctx *c, int n_agents, const srb12_sim *d, const srb12_plant *pl,
                                              int cycle, void *stream)
{
    return sim12_call<true>(c, n_agents, d, cycle, stream, nullptr, nullptr, pl);
}

extern "C" int srb12_sim_advance_device(srb12_ctx *c, int n_agents, const srb12_sim *d, int cycle, void *stream)
{
    return srb12_sim_advance_plant_device(c, n_agents, d, nullptr, cycle, stream);
}

extern "C" int srb12_sim_metrics_agents_device(srb12_ctx *c, int n_agents, const srb12_sim *d, const srb_sizes *sz,
                                               const srb_agent_sizes *ag, int cycle, void *stream)
{
    return sim12_call<false>(c, n_agents, d, cycle, stream, sz, ag, nullptr);
}

extern "C" int srb12_sim_metrics_sized_device(srb12_ctx *c, int n_agents, const srb12_sim *d, const srb_sizes *sz,
                                              int cycle, void *stream)
{
    return srb12_sim_metrics_agents_device(c, n_agents, d, sz, nullptr, cycle, stream);
}

extern "C" int srb12_sim_metrics_device(srb12_ctx *c, int n_agents, const srb12_sim *d, int cycle, void *stream)
{
    return srb12_sim_metrics_sized_device(c, n_agents, d, nullptr, cycle, stream);
}

// the shift of the plans (srb12_plan_shift_kernel): launch only, the caller orders the stream
static int launch_shift12(srb12_ctx *c, int n_agents, const double *plan, int grids, double *table, hipStream_t s)
{
    const int threads = n_agents * c->p.N;                // one per (agent, grid), as the advance
    hipLaunchKernelGGL(srb12_plan_shift_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, n_agents, c->p.N, grids, plan,
                       table);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

extern "C" int srb12_shift_plans_device(srb12_ctx *c, int n_agents, const double *plan, int grids, double *table,
                                        void *stream)
{
    if (grids < 0) return srb_internal_fail(SRB_ERR_ARG, "srb12_shift_plans_device: grids must be >= 0");
    if (!plan || !table) return srb_internal_fail(SRB_ERR_ARG, "srb12_shift_plans_device: missing buffer (plan, table)");
    if (plan == table) return srb_internal_fail(SRB_ERR_ARG, "srb12_shift_plans_device: plan and table must be two buffers");
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (c->p.N < 2) return srb_internal_fail(SRB_ERR_ARG, "srb12_shift_plans_device needs N >= 2 (the last finite difference)");
    if (n_agents < 0 || n_agents > c->max_agents) return srb_internal_fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (srb_overlap(plan, (size_t)n_agents * 2 * c->p.N, table, (size_t)n_agents * 2 * c->p.N))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_shift_plans_device: plan and table overlap");
    if (n_agents == 0) return SRB_OK;
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] { return launch_shift12(c, n_agents, plan, grids, table, s); });
}

extern "C" int srb12_obstacles_advance_device(srb12_ctx *c, int n_obs, double *obstacles, const double *obs_vel, void *stream)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    if (n_obs < 0) return srb_internal_fail(SRB_ERR_ARG, "srb12_obstacles_advance_device: negative n_obs");
    if (n_obs == 0) return SRB_OK;
    if (!obstacles || !obs_vel)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_obstacles_advance_device: obstacles / obs_vel missing");
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] { return srb_launch_obstacles_advance(n_obs, c->p.Ts, obstacles, obs_vel, s); });
}

// ---- degraded neighbour link (srb_link, srb_link.hip): the LIP mode's struct, checks and kernel.  The snapshot row
// last_state [A][4] and the plan tables [A][N][2] have the LIP layouts and one cycle is 4 grids in both modes; N and
// Ts are this context's (the selection context's are placeholders).  The argument errors that need the context:
// the plan ranges (N).  plan: the solve's plan output (srb12_plans.plan) or null
static int check_link_ctx12(const srb12_ctx *c, const srb_link *ln, int n_all, const double *plan_table, const double *plan)
{
    if (!srb_link_on(ln)) return SRB_OK;
    if (plan_table && c->p.N < 2) return srb_internal_fail(SRB_ERR_ARG, "srb_link: a plan table needs N >= 2 (the plan shift)");
    const size_t rows = (size_t)(n_all > 0 ? n_all : 0) * 2 * c->p.N;
    if (srb_overlap(ln->seen_plan, rows, plan_table, rows))
        return srb_internal_fail(SRB_ERR_ARG, "srb_link.seen_plan overlaps plan_table (the truth the next cycle's messages "
                                              "carry: use two buffers)");
    if (srb_overlap(ln->seen_plan, rows, plan, rows))
        return srb_internal_fail(SRB_ERR_ARG, "srb_link.seen_plan overlaps srb12_plans.plan (the solve reads the table while "
                                              "it writes its plans: use two buffers)");
    return SRB_OK;
}

// one cycle's update (launch only: the caller orders the stream); ln is on
static int launch_link12(srb12_ctx *c, int n_all, const srb_link *ln, const double *last_state, const double *plan_table,
                         int cycle, int c_first, hipStream_t s)
{
    const int slot = (int)(((long long)cycle - c_first) % (ln->max_delay + 1));
    int *age_row = ln->age_log ? ln->age_log + (size_t)(cycle - c_first) * (size_t)n_all : nullptr;
    if (srb_launch_link_update(SRB_LINK_LANES, n_all, c->p.N, c->p.Ts, cycle, c_first, ln->max_delay, slot,
                               ln->extrapolate, (unsigned)(ln->seed & 0xffffffffull), (unsigned)(ln->seed >> 32),
                               ln->delay, ln->drop, ln->noise_p, ln->noise_v, last_state, plan_table, ln->ring_state,
                               ln->ring_plan, ln->held_state, ln->held_plan, ln->held_cycle, ln->seen_state,
                               ln->seen_plan, age_row, s))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_link_update_device: no such thread mapping");
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

extern "C" int srb12_link_update_device(srb12_ctx *c, int n_all, const srb_link *ln, const double *last_state,
                                        const double *plan_table, int cycle, int c_first, void *stream)
{
    if (int rc = srb_check_link(ln, n_all, last_state, plan_table)) return rc;
    if (cycle < c_first) return srb_internal_fail(SRB_ERR_ARG, "srb_link: cycle precedes c_first");
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (n_all < 0) return srb_internal_fail(SRB_ERR_ARG, "srb_link: negative n_all");
    if (int rc = check_link_ctx12(c, ln, n_all, plan_table, nullptr)) return rc;
    if (!srb_link_on(ln) || n_all == 0) return SRB_OK;
    if (!last_state) return srb_internal_fail(SRB_ERR_ARG, "srb_link: last_state missing");
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] { return launch_link12(c, n_all, ln, last_state, plan_table, cycle, c_first, s); });
}

// pl: the plans fed forward (srb12_rollout_plans_device), or NULL (srb12_rollout_device: today's launches); mv: the
// moving obstacles (srb12_rollout_moving_device), or NULL; sz: the obstacle sizes (srb12_rollout_sized_device), or
// NULL; ag: the agent sizes (srb12_rollout_agents_device), or NULL; pt: the disturbed plant
// (srb12_rollout_plant_device), or NULL; ln: the degraded link (srb12_rollout_link_device), or NULL -- the tables do
// not change over a rollout: the same pointers serve every cycle
// (Every rollout entry point comes this way: one path.)
extern "C" int srb12_rollout_link_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                         const srb12_plans *pl, const srb_moving *mv, const srb_sizes *sz,
                                         const srb_agent_sizes *ag, const srb12_plant *pt, const srb_link *ln, int cycles,
                                         void *stream)
{
    if (int rc = srb_check_struct(b, "srb12_batch")) return rc;
    if (int rc0 = check_tables12(mv, sz, ag, b, true)) return rc0;
    if (int rc0 = check_plant12(pt, nullptr)) return rc0;         // (a missing buffer of the roll is reported below, as ever)
    if (!plant12_on(pt)) pt = nullptr;
    if (int rc = srb_check_struct(pl, "srb12_plans")) return rc;
    // (the layout and null checks of check_sim12 only: the driver's first cycle is c_first itself)
    if (int rc = check_sim12(d, d && d->struct_size == (int)sizeof(srb12_sim) ? d->c_first : 0, false)) return rc;
    // (the truth plan table of the link is the plans' plan_table, whose struct_size was checked above)
    if (int rc0 = srb_check_link(ln, n_agents, d->last_state, pl ? pl->plan_table : nullptr)) return rc0;
    if (!b) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (!d->goal) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim.goal missing");
    if (pl)
        if (int rc = check_plans12(b, pl, true)) return rc;
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    if (cycles < 0) return srb_internal_fail(SRB_ERR_ARG, "negative cycles");
    if (n_agents < 0 || n_agents > c->max_agents) return srb_internal_fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (b->agent_offset != 0 || d->agent_offset != 0 || (b->n_all != 0 && b->n_all != n_agents) ||
        (d->n_all != 0 && d->n_all != n_agents))
        return srb_internal_fail(SRB_ERR_ARG, "srb12_rollout_device rolls out a whole team on one GPU: a sharded batch "
                                              "(agent_offset != 0 or n_all != n_agents) needs the neighbour exchange "
                                              "between advance and metrics");
    if (int rc0 = check_link_ctx12(c, ln, n_agents, pl ? pl->plan_table : nullptr, pl ? pl->plan : nullptr)) return rc0;
    if (srb_link_on(ln) && pl && pl->plan_selection)      // (the selection's own plan will be the truth plan_table)
        if (int rc0 = check_own_plan12(pl->plan_table, pl, ag)) return rc0;
    if (!srb_link_on(ln)) ln = nullptr;
    int sa = 0, so = 0;
    if (int rc = srb_ctx_scenes(c->sel_ctx, &sa, &so)) return rc;
    if (sa > 0) {
        if (n_agents % sa != 0)
            return srb_internal_fail(SRB_ERR_ARG, ("scenes: srb12_rollout_device rolls out whole scenes, n_agents (" +
                                                   std::to_string(n_agents) + ") is not a multiple of scene_agents (" +
                                                   std::to_string(sa) + ")").c_str());
        if (int rc = srb_internal_check_scenes(c->sel_ctx, n_agents, b->n_obs, true, n_agents, 0)) return rc;
    }
    if (n_agents == 0) return SRB_OK;
    // the two structs wired together (include/srbnmpc.h): the solve reads what the advance wrote and back
    srb12_sim sim = *d;
    sim.x = b->x; sim.status = b->status; sim.iters = b->iters;
    sim.obstacles = b->obstacles; sim.n_obs = b->n_obs;
    sim.nbr_state = d->last_state; sim.n_all = n_agents; sim.agent_offset = 0;
    srb12_batch bat = *b;
    bat.x0 = d->x0; bat.xref = d->xref; bat.foot = d->foot; bat.contact = d->contact;
    bat.nbr_state = d->last_state; bat.n_all = n_agents; bat.agent_offset = 0;
    if (ln) bat.nbr_state = ln->seen_state;               // the solve reads what is seen, the metrics the truth
    if (!b->x || !b->obj || !b->status || !b->iters)
        return srb_internal_fail(SRB_ERR_ARG, "srb12_batch: missing buffer (x, obj, status, iters)");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    int rc = c->order.order_after_last(s);
    if (rc) return rc;
    // moving obstacles: the table advances one cycle between the agents' advance and the metrics, from the second
    // cycle on, so d_obs / fail_cycle and the solve see the agents and the obstacles at matching times
    SrbTables t = srb_tables(mv, sz, ag);
    if (b->n_obs <= 0) { t.obs_vel = nullptr; t.normalise(); }   // (no rows: nothing moves)
    for (int i = 0; i <= cycles && !rc; i++) {
        const int cyc = d->c_first + i;
        rc = launch_advance12(c, n_agents, &sim, cyc, s, pt);
        if (rc || i == cycles) break;
        if (i > 0 && t.obs_vel) rc = srb_launch_obstacles_advance(b->n_obs, c->p.Ts, mv->obstacles, t.obs_vel, s);
        if (!rc) rc = launch_metrics12(c, n_agents, &sim, cyc, s, t);
        if (!rc && ln) rc = launch_link12(c, n_agents, ln, d->last_state, pl ? pl->plan_table : nullptr, cyc, d->c_first, s);
        if (!pl) {
            if (!rc) rc = launch12(c, n_agents, &bat, s, nullptr, t);
            continue;
        }
        // the first solve against the caller's table (or none), every later one against last cycle's shifted plans
        // (under a link the perceived table; the selection then takes the agent's own plan from the truth)
        srb12_plans cur = *pl;
        if (i > 0) cur.nbr_plan = ln ? ln->seen_plan : pl->plan_table;
        if (!cur.nbr_plan) cur.plan_selection = 0;
        const double *own = (ln && i > 0 && cur.plan_selection) ? pl->plan_table : nullptr;
        if (!rc) rc = launch12(c, n_agents, &bat, s, &cur, t, own);
        if (!rc) rc = launch_shift12(c, n_agents, pl->plan, SRB12_SIM_NDOMAIN, pl->plan_table, s);
    }
    const int rc_mark = c->order.mark_done(s);            // also after a refusal inside the loop: earlier cycles run
    return rc ? rc : rc_mark;
}

extern "C" int srb12_rollout_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d, int cycles,
                                    void *stream)
{
    return srb12_rollout_sized_device(c, n_agents, b, d, nullptr, nullptr, nullptr, cycles, stream);
}

extern "C" int srb12_rollout_plans_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                          const srb12_plans *pl, int cycles, void *stream)
{
    if (!pl) {      // this entry point needs its struct: the driver's refusals that stand before that one, then it
        if (int rc = srb_check_struct(b, "srb12_batch")) return rc;
        if (int rc = check_sim12(d, d && d->struct_size == (int)sizeof(srb12_sim) ? d->c_first : 0, false)) return rc;
        if (b && !d->goal) return srb_internal_fail(SRB_ERR_ARG, "srb12_sim.goal missing");
        return srb_internal_fail(SRB_ERR_ARG, "null argument");
    }
    return srb12_rollout_sized_device(c, n_agents, b, d, pl, nullptr, nullptr, cycles, stream);
}

// pl may be NULL (srb12_rollout_device with the table moved), else srb12_rollout_plans_device with it
extern "C" int srb12_rollout_moving_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                           const srb12_plans *pl, const srb_moving *mv, int cycles, void *stream)
{
    return srb12_rollout_sized_device(c, n_agents, b, d, pl, mv, nullptr, cycles, stream);
}

// pl and mv may be NULL, as in srb12_rollout_moving_device; sz NULL (or without a table): that entry point itself
extern "C" int srb12_rollout_sized_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                          const srb12_plans *pl, const srb_moving *mv, const srb_sizes *sz, int cycles,
                                          void *stream)
{
    return srb12_rollout_agents_device(c, n_agents, b, d, pl, mv, sz, nullptr, cycles, stream);
}

// pl, mv and sz may be NULL, as in srb12_rollout_sized_device; ag NULL (or without a table): that entry point itself
extern "C" int srb12_rollout_agents_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                           const srb12_plans *pl, const srb_moving *mv, const srb_sizes *sz,
                                           const srb_agent_sizes *ag, int cycles, void *stream)
{
    return srb12_rollout_plant_device(c, n_agents, b, d, pl, mv, sz, ag, nullptr, cycles, stream);
}

// pl, mv, sz and ag may be NULL, as in srb12_rollout_agents_device; pt NULL (or with nothing set): that entry point itself
extern "C" int srb12_rollout_plant_device(srb12_ctx *c, int n_agents, const srb12_batch *b, const srb12_sim *d,
                                          const srb12_plans *pl, const srb_moving *mv, const srb_sizes *sz,
                                          const srb_agent_sizes *ag, const srb12_plant *pt, int cycles, void *stream)
{
    return srb12_rollout_link_device(c, n_agents, b, d, pl, mv, sz, ag, pt, nullptr, cycles, stream);
}

// diagnostics (not in the public header): agent >= 0 records a per-iteration trace on the next
// calls (|r_d|, its threshold, |r_p|, mu, ap, ad, delta, sigma per iteration, QP then NLP);
// out != NULL copies the last trace [2][64][8] + 16 phase-cycle sums (-DSRB12_STAMPS builds) to the host
extern "C" int srb12_debug_trace(srb12_ctx *c, int agent, double *out)
{
    if (!c) return srb_internal_fail(SRB_ERR_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    if (out) {
        if (int rc = c->order.wait_idle()) return rc;
        HIPCHK(hipMemcpy(out, c->dbg, (2 * 64 * 8 + 16) * sizeof(double), hipMemcpyDeviceToHost));
    }
    c->dbg_agent = agent;
    HIPCHK(hipMemset(c->dbg, 0, SRB12_DBG_LEN * sizeof(double)));
    return SRB_OK;
}

// diagnostics (not in the public header): the 128 state checks of the traced agent that a -DSRB12_CHECK
// build records in its polish (srb12_kernels.hip S12CK; tools/srb12_check.py); zeros in other builds
extern "C" int srb12_debug_check(srb12_ctx *c, double *out)
{
    if (!c || !out) return srb_internal_fail(SRB_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if (int rc = c->order.wait_idle()) return rc;
    HIPCHK(hipMemcpy(out, c->dbg + (2 * 64 * 8 + 16), 128 * sizeof(double), hipMemcpyDeviceToHost));
    return SRB_OK;
}
