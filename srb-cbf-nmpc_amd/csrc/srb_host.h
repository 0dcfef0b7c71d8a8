// Host plumbing shared by the three C-ABI files (srb_capi.cpp, srb12_capi.cpp, srb_ll_capi.cpp): the error
// channel, the HIP-error macros, the submission-order chaining of a context, and what the LIP and the SRB-12 mode
// check and launch alike (the struct-size refusal, the range-overlap test, the srb_moving, srb_sizes and srb_agent_sizes
// checks, the two values that carry the optional tables and a selection past those checks -- SrbTables, SrbSelect --
// the staging of a host table, the obstacle-advance launch).  Internal, host only.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "srbnmpc.h"
#include "srb_kernel_decls.h"

// What the launches need of the three optional structs (srb_moving, srb_sizes, srb_agent_sizes; each may be null),
// resolved once by srb_tables() below.  A new table is a new member here, not a new argument of every launcher.
struct SrbTables {
    const double *obs_vel;         // srb_moving.obs_vel [n_obs][2] (null: static obstacles, every launch as without)
    int obs_horizon;               // ... horizon_selection: the static columns by closest predicted approach
    const double *obs_eps;         // srb_sizes.obs_eps [n_obs] (null: eps_obs for every row)
    int obs_clear;                 // ... clearance_selection: the static columns by clearance to the level set
    const double *agent_rad, *agent_pad;   // srb_agent_sizes [n_all] each (null: eps_nbr and the levels as they are)
    int nbr_clear;                 // ... clearance_selection: the neighbour columns by clearance
    // the drivers' metrics: srb_sizes.obs_radius (null: centre distances and the 0.5 m fail test), srb_agent_sizes
    // .agent_body and its collide_cycle (body null: d_agent by centres)
    const double *obs_radius, *agent_body;
    int *collide_cycle;
    // a flag whose table is null is 0 (the selection ignores such a flag anyway: srb_internal_select)
    void normalise()
    {
        if (!obs_vel) obs_horizon = 0;
        if (!obs_eps) obs_clear = 0;
        if (!agent_rad) nbr_clear = 0;
    }
    // What a solve kernel is handed: vel, eps and pad are read for the static columns of sel only, rad for the
    // neighbour columns only (obs_rows, nbr_rows: the NLP stage has such columns after the clamp)
    SrbTables gated(bool obs_rows, bool nbr_rows) const
    {
        SrbTables g = *this;
        if (!obs_rows) g.obs_vel = g.obs_eps = g.agent_pad = nullptr;
        if (!nbr_rows) g.agent_rad = nullptr;
        g.normalise();
        return g;
    }
    bool any_solve_table() const { return obs_vel || obs_eps || agent_rad || agent_pad; }
};

static inline SrbTables srb_tables(const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag)
{
    SrbTables t = {};
    if (mv) { t.obs_vel = mv->obs_vel; t.obs_horizon = mv->horizon_selection; }
    if (sz) { t.obs_eps = sz->obs_eps; t.obs_clear = sz->clearance_selection; t.obs_radius = sz->obs_radius; }
    if (ag) {
        t.agent_rad = ag->agent_rad; t.agent_pad = ag->agent_pad; t.nbr_clear = ag->clearance_selection;
        t.agent_body = ag->agent_body; t.collide_cycle = ag->collide_cycle;
    }
    t.normalise();
    return t;
}

// One selection: what srb_internal_select and the launchers under it share.  K_obs, K_nbr are already clamped to
// the tables; x0 rows are [x, ., y, .] (stride 4).  Row a of sel holds the static columns 0 .. K_obs - 1, then the
// neighbour columns.  Callers start from SrbSelect{} and assign the members by name.
struct SrbSelect {
    int n_agents;
    const double *x0;
    int agent_offset;
    const double *obstacles;       // [n_obs][2]; obstacles_version != 0: a static table that keeps its grid
    int n_obs, obstacles_version;
    const double *nbr_state;       // [n_all][4]
    int n_all;
    int K_obs, K_nbr;
    int *sel;
    int sel_stride;                // 0: K_obs + K_nbr
    hipStream_t s;
    int N;                         // the horizon's grid (N, Ts) of the plan, horizon and clearance selections
    double Ts;
    const double *nbr_plan;        // [n_all][N][2] != null: the neighbour columns by closest predicted approach
    const double *own_plan;        // [n_agents][N][2] with nbr_plan: the agent's own plan there, not row g of the table
    SrbTables t;
    int stride() const { return sel_stride ? sel_stride : K_obs + K_nbr; }
    // the passes over one side alone, into the same rows of sel
    SrbSelect obs_only() const
    {
        SrbSelect q = *this;
        q.sel_stride = stride();
        q.nbr_state = nullptr; q.n_all = 0; q.K_nbr = 0;
        return q;
    }
    SrbSelect nbr_only() const     // (sel then points at the neighbour columns; no grid of the static table is kept)
    {
        SrbSelect q = *this;
        q.sel_stride = stride(); q.sel = sel + K_obs;
        q.n_obs = 0; q.obstacles_version = 0; q.K_obs = 0;
        return q;
    }
};

// defined in srb_capi.cpp: the thread's last-error message (srb_last_error), and the LIP-mode context's selection
// launch (q.t with its flags: the static columns by srb_moving.horizon_selection or srb_sizes.clearance_selection, the
// neighbour columns by srb_agent_sizes.clearance_selection; q.nbr_plan: the neighbour columns by the horizon-aware
// selection of SRB_OPT_PLAN_SELECTION, whatever that option of the context says) and ordering mark, which the SRB-12
// mode reuses
int srb_internal_fail(int code, const char *msg);
int srb_internal_select(srb_ctx *c, const SrbSelect &q);
int srb_internal_mark_done(srb_ctx *c, hipStream_t s);
// ... and its scene partition (srb_ctx_set_scenes): the per-call refusals, the "up to K nearest" clamp, and the
// metrics launch (srb_sim_metrics_kernel, or with scenes srb_sim_scene_metrics_kernel) on d->state rows
// [x, xdot, y, ydot] -- launches only, the caller orders the stream.  t.obs_radius: the sized kernels of
// srb_sizes.hip; t.agent_body (and t.collide_cycle): the kernels of srb_agents.hip
int srb_internal_check_scenes(const srb_ctx *c, int n_agents, int n_obs, bool has_nbr, int n_all, int agent_offset);
void srb_internal_clamp_K(const srb_ctx *c, int n_obs, bool has_nbr, int n_all, int *Ko, int *Kn);
int srb_internal_sim_metrics(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, hipStream_t s, const SrbTables &t);

// a failed HIP call returns SRB_ERR_HIP with "<expression>: <HIP's message>"; HIPCHK_UNWIND_ first runs `cleanup`
// (a create function's local CREATE_CHK names its destroy there once).  `text`: the expression stringified by the
// outermost macro, before the expression's own macros expand
#define HIPCHK(expr) HIPCHK_UNWIND_(expr, #expr, (void)0)
#define HIPCHK_UNWIND(expr, cleanup) HIPCHK_UNWIND_(expr, #expr, cleanup)
#define HIPCHK_UNWIND_(expr, text, cleanup)                                                                     \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            const int rc_ = srb_internal_fail(SRB_ERR_HIP, (std::string(text ": ") + hipGetErrorString(e_)).c_str()); \
            cleanup;                /* (a destroy function sets no error: the message above stays) */           \
            return rc_;                                                                                         \
        }                                                                                                       \
    } while (0)

// Calls on one context run in submission order (include/srbnmpc.h, "Ordering"): a call on another stream than
// the previous one first waits for that call's work, so the context's scratch (grids, the default sel buffer,
// staging, timing events) never serves two launches in flight.
struct SrbCallOrder {
    hipEvent_t done;               // recorded after every call's work
    hipStream_t last;              // stream of the previous call
    bool any;                      // a call has been submitted (done is valid)
    int order_after_last(hipStream_t s)
    {
        if (any && s != last) HIPCHK(hipStreamWaitEvent(s, done, 0));
        return SRB_OK;
    }
    int mark_done(hipStream_t s)
    {
        HIPCHK(hipEventRecord(done, s));
        last = s; any = true;
        return SRB_OK;
    }
    int wait_idle()                // the last call may be on another stream than the caller's
    {
        if (any) HIPCHK(hipEventSynchronize(done));
        return SRB_OK;
    }
    // One whole call: on `device`, `launch()` on s after the context's previous call, then the mark.  (The solves
    // and the rollout drivers differ -- no mark without agents, a mark after a refusal -- and spell it out.)
    template <class Launch> int run(int device, hipStream_t s, Launch launch)
    {
        HIPCHK(hipSetDevice(device));
        int rc = order_after_last(s);
        if (!rc) rc = launch();
        if (!rc) rc = mark_done(s);
        return rc;
    }
};

// The layout refusal of a struct that carries its size (x null: nothing to refuse here); `name`: the struct's.
// It needs no context, so every entry point runs it first (tests/test_abi.py reaches it without a GPU).
template <class T> static inline int srb_check_struct(const T *x, const char *name)
{
    if (!x || x->struct_size == (int)sizeof(T)) return SRB_OK;
    const std::string n(name);
    return srb_internal_fail(SRB_ERR_ARG,
                             (n + ".struct_size != sizeof(" + n + "): caller built against another ABI").c_str());
}

// [a, a + na) and [b, b + nb) share an element (a null range shares none)
static inline bool srb_overlap(const double *a, size_t na, const double *b, size_t nb)
{
    return a && b && a < b + nb && b < a + na;
}

// The argument errors of srb_moving that need no context, before anything is launched (b may be null: the caller
// reports that).  rollout: the driver moves the table, so it needs the writable pointer to batch.obstacles.
// Batch: srb_batch or srb12_batch; `entry`, `batch`: the names of the mode's moving rollout and of its batch struct.
template <class Batch>
static int srb_check_moving(const srb_moving *mv, const Batch *b, bool rollout, const char *entry, const char *batch)
{
    if (int rc = srb_check_struct(mv, "srb_moving")) return rc;
    if (!mv) return SRB_OK;
    if (mv->horizon_selection != 0 && mv->horizon_selection != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb_moving.horizon_selection: 0 (nearest now) or 1 (closest predicted "
                                              "approach)");
    if (mv->horizon_selection && !mv->obs_vel)
        return srb_internal_fail(SRB_ERR_ARG, "srb_moving.horizon_selection = 1 needs obs_vel (the horizon-aware selection "
                                              "reads the velocity table)");
    if (!mv->obs_vel || !b || b->struct_size != (int)sizeof(Batch)) return SRB_OK;
    if (b->obstacles_version != 0)
        return srb_internal_fail(SRB_ERR_ARG, "srb_moving.obs_vel with obstacles_version != 0: a kept selection grid of a "
                                              "moving table is stale (pass version 0)");
    if (rollout && !mv->obstacles)
        return srb_internal_fail(SRB_ERR_ARG, (std::string(entry) + ": srb_moving.obstacles missing (the driver moves the "
                                               "table in place)").c_str());
    if (rollout && mv->obstacles != b->obstacles)
        return srb_internal_fail(SRB_ERR_ARG, (std::string(entry) + ": srb_moving.obstacles is not " + batch + ".obstacles "
                                               "(the solve and the metrics read the table the driver moves)").c_str());
    return SRB_OK;
}

// The argument errors of srb_sizes, none of which needs a context, before anything is launched.  (obs_eps goes
// together with obstacles_version != 0: sizes do not stale a grid of centres, and the clearance selection consults
// no grid.)
static inline int srb_check_sizes(const srb_sizes *sz)
{
    if (int rc = srb_check_struct(sz, "srb_sizes")) return rc;
    if (!sz) return SRB_OK;
    if (sz->clearance_selection != 0 && sz->clearance_selection != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb_sizes.clearance_selection: 0 (the K_obs columns as ever) or 1 (by "
                                              "clearance to the level set)");
    if (sz->clearance_selection && !sz->obs_eps)
        return srb_internal_fail(SRB_ERR_ARG, "srb_sizes.clearance_selection = 1 needs obs_eps (the clearance selection "
                                              "reads the level table)");
    return SRB_OK;
}

// The argument errors of srb_agent_sizes, none of which needs a context, before anything is launched.  has_nbr: the
// call's batch (srb_batch, or srb_sim for the metrics) has a neighbour table, whose rows the tables follow.
static inline int srb_check_agent_sizes(const srb_agent_sizes *ag, bool has_nbr)
{
    if (int rc = srb_check_struct(ag, "srb_agent_sizes")) return rc;
    if (!ag) return SRB_OK;
    if (ag->clearance_selection != 0 && ag->clearance_selection != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes.clearance_selection: 0 (the K_nbr columns as ever) or 1 "
                                              "(by clearance dist - agent_rad)");
    if (ag->clearance_selection && !ag->agent_rad)
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes.clearance_selection = 1 needs agent_rad (the clearance "
                                              "selection reads the radius table)");
    if (ag->agent_rad && !has_nbr)
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes.agent_rad needs a neighbour table (nbr_state, n_all > 0): "
                                              "its rows are the table's");
    if (ag->agent_body && !has_nbr)
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes.agent_body needs a neighbour table (nbr_state, n_all > 0): "
                                              "its rows are the table's");
    if (ag->collide_cycle && !ag->agent_body)
        return srb_internal_fail(SRB_ERR_ARG, "srb_agent_sizes.collide_cycle needs agent_body (a collision is two bodies "
                                              "overlapping)");
    return SRB_OK;
}

// the batch has a neighbour table (what srb_agent_sizes.agent_rad / agent_body need)
template <class Batch> static inline bool srb_has_nbr(const Batch *b)
{
    return b && b->struct_size == (int)sizeof(Batch) && b->nbr_state && b->n_all > 0;
}

// The three checks above in the order every entry point runs them, after its own srb_check_struct(batch).  rollout:
// the driver's rules (srb_check_moving), and its neighbour table is the team itself.
template <class Batch>
static int srb_check_tables(const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, const Batch *b,
                            bool rollout, const char *entry, const char *batch)
{
    if (int rc = srb_check_moving(mv, b, rollout, entry, batch)) return rc;
    if (int rc = srb_check_sizes(sz)) return rc;
    return srb_check_agent_sizes(ag, rollout || srb_has_nbr(b));
}

// ---- degraded neighbour link (srb_link; srb_link.hip), both modes.  The struct degrades the link at all (else every
// entry point is the one it extends and nothing is launched; age_log alone is not written)
static inline bool srb_link_on(const srb_link *ln) { return ln && (ln->delay || ln->drop || ln->noise_p || ln->noise_v); }

// The argument errors of srb_link that need no context, before anything is launched.  last_state, plan_table: the
// truth tables of the call ([n_all][4]; [n_all][N][2] or null)
#define SRB_LINK_MAX_DELAY 16
static inline int srb_check_link(const srb_link *ln, int n_all, const double *last_state, const double *plan_table)
{
    if (int rc = srb_check_struct(ln, "srb_link")) return rc;
    if (!ln) return SRB_OK;
    if (ln->max_delay < 0 || ln->max_delay > SRB_LINK_MAX_DELAY)
        return srb_internal_fail(SRB_ERR_ARG, "srb_link.max_delay: 0 .. 16 (the ring holds max_delay + 1 cycles)");
    if (ln->extrapolate != 0 && ln->extrapolate != 1)
        return srb_internal_fail(SRB_ERR_ARG, "srb_link.extrapolate: 0 (the held message as it is) or 1 (dead-reckoned by its age)");
    if (!srb_link_on(ln)) return SRB_OK;
    if (!ln->ring_state || !ln->held_state || !ln->held_cycle || !ln->seen_state)
        return srb_internal_fail(SRB_ERR_ARG, "srb_link: a link that is on needs ring_state, held_state, held_cycle and seen_state");
    if (plan_table && (!ln->ring_plan || !ln->held_plan || !ln->seen_plan))
        return srb_internal_fail(SRB_ERR_ARG, "srb_link: a plan table needs ring_plan, held_plan and seen_plan");
    if (n_all > 0 && srb_overlap(ln->seen_state, (size_t)n_all * 4, last_state, (size_t)n_all * 4))
        return srb_internal_fail(SRB_ERR_ARG, "srb_link.seen_state overlaps last_state (the metrics read the truth while the "
                                              "solve reads what is seen: use two buffers)");
    return SRB_OK;
}

// A staging buffer of the host-buffer entry points grown to `bytes` (contents not kept).  The context's last call
// may still read the old buffer; and whatever fails, the context is left with no buffer and no capacity, never
// with a freed pointer that a later, smaller call would copy into and the destroy would free again.
template <class T> static int srb_stage_reserve(SrbCallOrder &order, T *&buf, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return SRB_OK;
    if (int rc = order.wait_idle()) return rc;
    T *old = buf;
    buf = nullptr; cap = 0;
    if (old) HIPCHK(hipFree(old));
    void *fresh = nullptr;                 // (a failed hipMalloc is not promised to leave its argument null)
    HIPCHK(hipMalloc(&fresh, bytes));
    buf = (T *)fresh; cap = bytes;
    return SRB_OK;
}

// A host table staged into such a buffer on s: reserve, then the copy (after a failure the context is as
// srb_stage_reserve leaves it)
template <class T>
static int srb_stage_copy(SrbCallOrder &order, T *&buf, size_t &cap, const T *host_src, size_t bytes, hipStream_t s)
{
    if (int rc = srb_stage_reserve(order, buf, cap, bytes)) return rc;
    HIPCHK(hipMemcpyAsync(buf, host_src, bytes, hipMemcpyHostToDevice, s));
    return SRB_OK;
}

// one control cycle of an obstacle table (srb_obstacles_advance_kernel: 4 grids of Ts): launch only, the caller
// orders the stream
static inline int srb_launch_obstacles_advance(int n_obs, double Ts, double *obstacles, const double *obs_vel, hipStream_t s)
{
    hipLaunchKernelGGL(srb_obstacles_advance_kernel, dim3((n_obs + 255) / 256), dim3(256), 0, s, n_obs, Ts, obstacles,
                       obs_vel);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}
