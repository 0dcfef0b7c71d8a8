// Host plumbing shared by the three C-ABI files (srb_capi.cpp, srb12_capi.cpp, srb_ll_capi.cpp): the error
// channel, the HIP-error macros and the submission-order chaining of a context.  Internal, host only.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "srbnmpc.h"

// defined in srb_capi.cpp: the thread's last-error message (srb_last_error), and the LIP-mode context's selection
// launch and ordering mark, which the SRB-12 mode reuses (nbr_plan [n_all][N][2] != NULL: the neighbour columns by
// the horizon-aware selection of SRB_OPT_PLAN_SELECTION, whatever that option of the context says; obs_vel
// [n_obs][2] with obs_horizon != 0: the static columns by srb_moving.horizon_selection over the grid (N, Ts))
int srb_internal_fail(int code, const char *msg);
int srb_internal_select(srb_ctx *c, int n_agents, const double *x0, const double *obstacles, int n_obs,
                        const double *nbr_state, int n_all, int agent_offset, int K_obs, int K_nbr,
                        int obstacles_version, int *sel, hipStream_t s, const double *nbr_plan = nullptr, int N = 0,
                        const double *obs_vel = nullptr, int obs_horizon = 0, double Ts = 0.0);
int srb_internal_mark_done(srb_ctx *c, hipStream_t s);
// ... and its scene partition (srb_ctx_set_scenes): the per-call refusals, the "up to K nearest" clamp, and the
// metrics launch (srb_sim_metrics_kernel, or with scenes srb_sim_scene_metrics_kernel) on d->state rows
// [x, xdot, y, ydot] -- launches only, the caller orders the stream
int srb_internal_check_scenes(const srb_ctx *c, int n_agents, int n_obs, bool has_nbr, int n_all, int agent_offset);
void srb_internal_clamp_K(const srb_ctx *c, int n_obs, bool has_nbr, int n_all, int *Ko, int *Kn);
int srb_internal_sim_metrics(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, hipStream_t s);

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
};
