// Host side of the C ABI declared in include/srbnmpc.h.
//
// The context owns device staging buffers sized for max_agents, one HIP stream and a
// pair of events around each kernel, so bench.py can time the kernels on the stream
// they actually run on.  Per-call work on the host is only the (tiny) LIP
// discretisation shared by every agent and the launch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include "srbnmpc.h"
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"
#include "srb_host.h"

typedef void (*srb_kernel_fn)(SrbKParams, int, const double *, const double *, const double *, const double *, int,
                              const double *, int, int, double *, double *, double *, int *, int *, const double *,
                              double *, const int *, float *, int, const double *, double *);
typedef void (*srb_polish_fn)(SrbKParams, int, const double *, const double *, const double *, const double *,
                              const double *, double *, double *, int *, const double *, double *, const int *,
                              const float *, int, const double *, double *);
// the table instances (srb_nmpc_kernel_mv_* / srb_polish_kernel_mv_*): further arguments, the velocity table of
// srb_moving, the level table of srb_sizes and the radius and pad tables of srb_agent_sizes (each may be null); the
// polish kernel also the agent_offset of the agent tables' own row
typedef void (*srb_kernel_mv_fn)(SrbKParams, int, const double *, const double *, const double *, const double *, int,
                                 const double *, int, int, double *, double *, double *, int *, int *, const double *,
                                 double *, const int *, float *, int, const double *, double *, const double *,
                                 const double *, const double *, const double *);
typedef void (*srb_polish_mv_fn)(SrbKParams, int, const double *, const double *, const double *, const double *,
                                 const double *, double *, double *, int *, const double *, double *, const int *,
                                 const float *, int, const double *, double *, const double *, const double *,
                                 const double *, const double *, int);
// (each kernel's name stands beside its pointer: srb_ctx_last_kernels reports the name of what was launched)
struct srb_instance {
    int nzl, ts, nw, nc, cc, kc;
    srb_kernel_fn fn; const char *fn_name;
    srb_polish_fn polish; const char *polish_name;
    srb_kernel_mv_fn fn_mv; const char *fn_mv_name;
    srb_polish_mv_fn polish_mv; const char *polish_mv_name;
};
// solve kernel (INFIX empty, or f32_) and polish kernel of one instance, then their moving-obstacle instances; the
// pointer and its name as a string come from the one pasted token (ENTRY_FN_), so the two cannot drift apart
#define ENTRY_FN_(f) f, #f
#define ENTRY_NMPC_(INFIX, NZL, TS, NW, NC, CC, KC) NZL, TS, NW, NC, CC, KC, ENTRY_FN_(srb_nmpc_kernel_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC)
#define ENTRY_POLISH_(NZL, TS, NW, NC, CC, KC) ENTRY_FN_(srb_polish_kernel_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC)
#define ENTRY_MV_(INFIX, NZL, TS, NW, NC, CC, KC) ENTRY_FN_(srb_nmpc_kernel_mv_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC)
#define ENTRY_POLISH_MV_(NZL, TS, NW, NC, CC, KC) ENTRY_FN_(srb_polish_kernel_mv_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC)
#define ENTRY_NMPC(...) {ENTRY_NMPC_(, __VA_ARGS__), ENTRY_POLISH_(__VA_ARGS__), ENTRY_MV_(, __VA_ARGS__), ENTRY_POLISH_MV_(__VA_ARGS__)},
#define ENTRY_F32(...) {ENTRY_NMPC_(f32_, __VA_ARGS__), nullptr, "", ENTRY_MV_(f32_, __VA_ARGS__), nullptr, ""},
static const srb_instance g_instances[] = {SRB_KERNEL_INSTANCES(ENTRY_NMPC)};
// the fp32-factor variant of an instance (SRB_OPT_KKT_FP32_MU > 0), or null; these entries carry no polish kernel
static const srb_instance g_instances_f32[] = {SRB_KF32_INSTANCES(ENTRY_F32)};
#undef ENTRY_NMPC
#undef ENTRY_F32
static const srb_instance *f32_variant(const srb_instance *in)
{
    for (const srb_instance &v : g_instances_f32)
        if (v.nzl == in->nzl && v.ts == in->ts && v.nw == in->nw && v.nc == in->nc && v.cc == in->cc && v.kc == in->kc) return &v;
    return nullptr;
}

// Waves per agent: small batches (up to one agent per CU) spread each agent over the four
// SIMDs of a CU (NW = 4) for latency; larger batches run one wave per agent so that agents,
// not waves of one agent, fill the SIMDs.
static int g_cu_count = 0;
static size_t g_lds_max = 160 * 1024;   // gfx950 LDS per CU; the device's sharedMemPerBlock once known
// Waves per agent: small batches (up to one agent per CU) spread each agent over the four
// SIMDs of a CU (NW = 4) for latency; larger batches run one wave per agent so that agents,
// not waves of one agent, fill the SIMDs -- except large problems (more than five row slots per
// lane with one wave, e.g. N = 20), where one wave spills its registers and two waves per agent
// are 1.8x faster (profiles/r01_nw_tuning.txt).  srb_ctx_set_waves overrides.  (No environment
// variable changes what the product library computes: every knob is a context setting.)
static int wanted_waves(int n_agents, int slots, int ctx_nw)
{
    if (ctx_nw == 1 || ctx_nw == 2 || ctx_nw == 4) return ctx_nw;
    if (g_cu_count > 0 && n_agents <= g_cu_count) return 4;
    return (slots > 5 * 64) ? 2 : 1;
}

static const srb_instance *pick_instance(const SrbKParams &k, int nw = 1, size_t lds_max = g_lds_max)
{
    const int S = srb_slots(k.N, k.C, k.K_obs + k.K_nbr);
    for (int pass = 0; pass < 3; pass++) {
        const int want = pass == 0 ? nw : pass == 1 ? (nw == 4 ? 2 : 1) : 1;
        for (const srb_instance &in : g_instances)
            if (in.nw == want && in.nzl >= k.nz && 64 * in.nw * in.ts >= S &&
                (in.nc == 0 || in.nc == k.N) && (in.cc == 0 || in.cc == k.C) &&
                (in.kc == 0 || in.kc == k.K_obs + k.K_nbr) &&
                (size_t)srb_lds_doubles(k, in.nzl, in.nw) * sizeof(double) <= lds_max)
                return &in;
    }
    return nullptr;
}

static thread_local std::string g_err;

static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// shared with srb12_capi.cpp and srb_ll_capi.cpp (srb_host.h, whose HIPCHK reports through it)
int srb_internal_fail(int code, const char *msg) { return fail(code, msg); }

struct srb_ctx {
    srb_params p;
    int max_agents, device;
    hipStream_t stream;
    hipEvent_t ev[4];
    SrbCallOrder order;            // submission-order chaining of the calls on this context
    // device staging
    double *x0, *ref, *foot, *obstacles, *nbr, *x_qp, *x, *obj, *abuf, *alpha;
    double *nbr_plan, *plan;       // neighbour plan table (staged), this batch's plans [max_agents][N][2]
    size_t cap_plan;               // (the cap_* of the staged tables are bytes: srb_stage_reserve)
    int plan_selection;            // SRB_OPT_PLAN_SELECTION: 1 neighbours by closest predicted approach
    int *status, *iters;
    int *sel;                      // [max_agents][2 SRB_KNN_MAX] selected obstacle / neighbour rows
    size_t cap_obs, cap_nbr;
    double *obs_vel;               // staged obstacle velocities (srb_solve_batch_moving)
    size_t cap_vel;
    double *obs_eps;               // staged obstacle levels (srb_solve_batch_sized)
    size_t cap_eps;
    double *agent_rad, *agent_pad; // staged agent tables (srb_solve_batch_agents)
    size_t cap_rad, cap_pad;
    float knn_ms, solve_ms;
    bool timed;
    int last_nw;
    int nw;                        // waves per agent forced by srb_ctx_set_waves (0: automatic)
    int qp_init;                   // QP starting point (srb_ctx_set_qp_init): 1 scaled (default), 0 iSWIFT
    // srb_ctx_set_option (SRB_OPT_*): the polish of the NLP result on/off, its penalty and waves per
    // agent, the selection-grid thresholds
    int polish, polish_waves, grid_min_rows, grid_min_rows_static, polish_fused;
    int last_polish;               // how the last launch polished: 0 no, 1 polish kernel, 2 fused
    const char *last_solve_name, *last_polish_name;   // the kernels the last launch ran (srb_ctx_last_kernels)
    int timing;                    // 1: HIP events around the kernels (srb_last_kernel_ms); 0: none
    int selection;                 // SRB_OPT_SELECTION: 1 the solve launches the selection, 0 the caller did
    int last_f32;                  // the last launch ran an fp32-factor instance (SRB_OPT_LAST_KKT_FP32, read only)
    double polish_rho;
    double qp_warm_tol;            // SRB_OPT_QP_WARM_TOL
    double kkt32_mu;               // SRB_OPT_KKT_FP32_MU: fp32 factor while mu > this (0: off, the fp64 instances)
    int kkt32_ref;                 // SRB_OPT_KKT_FP32_REFINE: fp64 refinement steps per solve with the fp32 factor
    float *zpol;                   // [max_agents][zstride] NLP active set / multipliers for the polish kernel
    int zstride;
    float polish_ms;
    // selection grids (table 0: static obstacles, 1: neighbour snapshot), rebuilt per launch
    struct grid_buf { SrbGrid *g; int *off; double2 *spos; int *sidx; size_t cap; } grid[2];
    const double *grid_src;        // obstacle table, row count and version the obstacle grid was built from
    int grid_n, grid_ver;
    int scene_agents, scene_obs;   // srb_ctx_set_scenes: agents / obstacle rows per scene (0, 0: one team)
};

// device buffers of selection grid t for a table of n rows (grown on demand; the header
// starts with ok = 0, so a grid is never read before a build has filled it)
static int grid_reserve(srb_ctx *c, int t, size_t n)
{
    srb_ctx::grid_buf &b = c->grid[t];
    if (!b.g) {
        HIPCHK(hipMalloc(&b.g, 64));
        HIPCHK(hipMemset(b.g, 0, 64));
        HIPCHK(hipMalloc(&b.off, (SRB_GRID_CELLS + 1) * sizeof(int)));
    }
    if (n > b.cap) {
        if (int rc = c->order.wait_idle()) return rc;       // the previous launch may still read them
        if (b.spos) HIPCHK(hipFree(b.spos));
        if (b.sidx) HIPCHK(hipFree(b.sidx));
        HIPCHK(hipMalloc(&b.spos, n * sizeof(double2)));
        HIPCHK(hipMalloc(&b.sidx, n * sizeof(int)));
        b.cap = n;
    }
    return SRB_OK;
}

extern "C" void srb_params_default(srb_params *p, int N, int C)
{
    std::memset(p, 0, sizeof(*p));
    p->N = N; p->C = C; p->K_obs = 1; p->K_nbr = 0;
    p->grav = 9.81; p->hcom = 0.29; p->Ts = 43 * 0.001; p->mu = 0.7;
    p->Qw = 3e2; p->Pw = 2e3; p->Rw = 1e-1; p->Sw = 0.3e4;
    p->box = 1e3;
    p->eps_obs = (double)1.9f; p->eps_nbr = (double)2.2f; p->vsat = (double)0.35f;
    p->tol = 1e-6; p->qp_maxit = 25; p->nlp_maxit = 50; p->use_nlp = 1;
}

extern "C" int srb_nv(const srb_params *p) { return (6 + p->C) * p->N + 1; }

extern "C" int srb_abi_version(void) { return SRB_ABI_VERSION; }

static void mm4(const double *X, const double *Y, double *Z)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += X[i * 4 + k] * Y[k * 4 + j];
            Z[i * 4 + j] = s;
        }
}

// Inverse of the 5x5 Bernstein matrix B[i][j] = C(4,j) s_i^j (1-s_i)^(4-j), s_i = i/4
// (fitComTrajectory_eventbase, MPC_dist.cpp:801-806), Gauss-Jordan with partial pivoting.
static void bernstein_inverse(double Binv[25])
{
    static const double binom[5] = {1, 4, 6, 4, 1};
    double M[5][10];
    for (int i = 0; i < 5; i++) {
        const double s = i * 0.25;
        for (int j = 0; j < 5; j++) { M[i][j] = binom[j] * std::pow(s, j) * std::pow(1 - s, 4 - j); M[i][5 + j] = (i == j); }
    }
    for (int k = 0; k < 5; k++) {
        int piv = k;
        for (int i = k + 1; i < 5; i++) if (std::fabs(M[i][k]) > std::fabs(M[piv][k])) piv = i;
        for (int j = 0; j < 10; j++) std::swap(M[k][j], M[piv][j]);
        const double inv = 1.0 / M[k][k];
        for (int j = 0; j < 10; j++) M[k][j] *= inv;
        for (int i = 0; i < 5; i++)
            if (i != k) {
                const double f = M[i][k];
                for (int j = 0; j < 10; j++) M[i][j] -= f * M[k][j];
            }
    }
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) Binv[i * 5 + j] = M[i][5 + j];
}

// LIP discretisation MPC_dist.cpp:99-127 (Ad by third-order series, Bd = A^-1 (Ad - I) B)
static SrbKParams make_kparams(const srb_params *p, int use_nlp)
{
    SrbKParams k;
    std::memset(&k, 0, sizeof k);
    k.N = p->N; k.C = p->C; k.K_obs = p->K_obs; k.K_nbr = p->K_nbr;
    k.n = (6 + p->C) * p->N + 1;
    k.nz = p->N * (p->C - 1) + 1;
    k.mq = 4 * (p->N - 1) + 12 * p->N + 2 * p->C * p->N;
    k.use_nlp = use_nlp;
    k.qp_maxit = p->qp_maxit; k.nlp_maxit = p->nlp_maxit;
    const double w2 = p->grav / p->hcom, T = p->Ts;
    double A[16] = {0}, B[8] = {0}, A2[16], A3[16];
    A[1] = 1; A[4] = w2; A[11] = 1; A[14] = w2;
    B[2] = -w2; B[7] = -w2;
    mm4(A, A, A2); mm4(A2, A, A3);
    for (int i = 0; i < 16; i++) k.Ad[i] = (i % 5 == 0 ? 1.0 : 0.0) + A[i] * T + 0.5 * A2[i] * T * T + A3[i] * T * T * T / 6;
    double Ai[16] = {0}, AdI[16], M[16];
    Ai[1] = 1.0 / w2; Ai[4] = 1.0; Ai[11] = 1.0 / w2; Ai[14] = 1.0;
    for (int i = 0; i < 16; i++) AdI[i] = k.Ad[i] - (i % 5 == 0 ? 1.0 : 0.0);
    mm4(Ai, AdI, M);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 2; j++) {
            double s = 0;
            for (int q = 0; q < 4; q++) s += M[i * 4 + q] * B[q * 2 + j];
            k.Bd[i * 2 + j] = s;
        }
    k.Qw = p->Qw; k.Pw = p->Pw; k.Rw = p->Rw; k.Sw = p->Sw; k.box = p->box;
    k.fr = p->mu * p->hcom / std::sqrt(2.0);
    k.eps_obs = p->eps_obs; k.eps_nbr = p->eps_nbr; k.vsat = p->vsat; k.tol = p->tol; k.Ts = p->Ts;
    bernstein_inverse(k.Binv);
    return k;
}

static int validate(const srb_params *p)
{
    if (!p) return fail(SRB_ERR_ARG, "null params");
    if (p->N < 2 || p->C < 2 || p->C > 4) return fail(SRB_ERR_ARG, "need N >= 2 and 2 <= C <= 4");
    if (p->N > SRB_MAX_N) return fail(SRB_ERR_SIZE, "N exceeds 33 (CoM-CoP slots in one 64-lane trip)");
    if (p->K_obs < 0 || p->K_nbr < 0 || p->K_obs > SRB_KNN_MAX || p->K_nbr > SRB_KNN_MAX)
        return fail(SRB_ERR_ARG, "K_obs, K_nbr out of range (each <= 16)");
    if (p->N * (p->C - 1) + 1 > SRB_MAX_NZ) return fail(SRB_ERR_SIZE, "N(C-1)+1 exceeds 32 (reduced Newton system bound)");
    SrbKParams k = make_kparams(p, p->use_nlp);
    const srb_instance *in = pick_instance(k);
    if (!in) return fail(SRB_ERR_SIZE, "no kernel instance covers the row slots (n + 4N - 2 + N K <= 512)");
    if ((size_t)srb_lds_doubles(k, in->nzl, in->nw) * sizeof(double) > 160 * 1024) return fail(SRB_ERR_SIZE, "per-agent LDS exceeds 160 KiB");
    return SRB_OK;
}

// the parameter checks of srb_ctx_create alone (no device needed)
extern "C" int srb_check_params(const srb_params *p) { return validate(p); }

extern "C" int srb_lds_bytes(const srb_params *p)
{
    SrbKParams k = make_kparams(p, p->use_nlp);
    const srb_instance *in = pick_instance(k);
    return in ? srb_lds_doubles(k, in->nzl, in->nw) * (int)sizeof(double) : -1;
}

extern "C" int srb_ctx_create(const srb_params *p, int max_agents, int device, srb_ctx **out)
{
    if (!out || max_agents <= 0) return fail(SRB_ERR_ARG, "bad arguments");
    int rc = validate(p);                 // parameter checks first (no device needed)
    if (rc) return rc;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SRB_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    if (g_cu_count == 0) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        g_cu_count = prop.multiProcessorCount;
        g_lds_max = prop.sharedMemPerBlock;
    }
    rc = validate(p);                     // again against this device's LDS per workgroup
    if (rc) return rc;
    srb_ctx *c = new srb_ctx();           // value-initialised: every buffer null until allocated
    // a failure after this point unwinds through srb_ctx_destroy; *out stays untouched
    c->p = *p; c->max_agents = max_agents; c->device = device;
    c->cap_obs = 0; c->cap_nbr = 0; c->obstacles = nullptr; c->nbr = nullptr; c->timed = false; c->nw = 0; c->last_nw = 0;
    for (auto &g : c->grid) g = srb_ctx::grid_buf{nullptr, nullptr, nullptr, nullptr, 0};
    c->grid_src = nullptr; c->grid_n = 0; c->grid_ver = 0;
    c->qp_init = 1; c->polish_ms = 0.0f;
    c->polish = 1; c->polish_rho = SRB_POLISH_RHO; c->qp_warm_tol = SRB_QP_WARM_TOL; c->polish_waves = 0; c->polish_fused = 1; c->last_polish = 0; c->last_solve_name = ""; c->last_polish_name = ""; c->timing = 1; c->selection = 1;
    c->kkt32_mu = 0.0; c->kkt32_ref = 3;
    c->nbr_plan = nullptr; c->cap_plan = 0; c->plan_selection = 0;
    c->grid_min_rows = SRB_GRID_MIN_ROWS; c->grid_min_rows_static = SRB_GRID_MIN_ROWS_STATIC;
    c->zstride = 2 * srb_r4(srb_slots(p->N, p->C, p->K_obs + p->K_nbr));
    const int N = p->N, C = p->C, nv = srb_nv(p);
    const size_t A = (size_t)max_agents;
#define CREATE_CHK(expr) HIPCHK_UNWIND_(expr, #expr, srb_ctx_destroy(c))
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) CREATE_CHK(hipEventCreate(&c->ev[i]));
    CREATE_CHK(hipEventCreateWithFlags(&c->order.done, hipEventDisableTiming));
    CREATE_CHK(hipMalloc(&c->x0, A * 4 * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->ref, A * 4 * N * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->foot, A * 2 * C * N * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->x_qp, A * nv * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->x, A * nv * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->obj, A * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->status, A * 2 * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->iters, A * 2 * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->abuf, A * 4 * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->alpha, A * 20 * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->plan, A * 2 * N * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->sel, A * 2 * SRB_KNN_MAX * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->zpol, A * (size_t)c->zstride * sizeof(float)));
#undef CREATE_CHK
    *out = c;
    return SRB_OK;
}

extern "C" int srb_ctx_destroy(srb_ctx *c)
{
    if (!c) return SRB_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)c->order.wait_idle();                         // the last launch may be on another stream
    void *bufs[] = {c->x0, c->ref, c->foot, c->x_qp, c->x, c->obj, c->status, c->iters, c->obstacles, c->nbr,
                    c->abuf, c->alpha, c->sel, c->zpol, c->nbr_plan, c->plan, c->obs_vel, c->obs_eps,
                    c->agent_rad, c->agent_pad};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    for (auto &g : c->grid)
        for (void *b : {(void *)g.g, (void *)g.off, (void *)g.spos, (void *)g.sidx})
            if (b) (void)hipFree(b);
    for (int i = 0; i < 4; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->order.done) (void)hipEventDestroy(c->order.done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SRB_OK;
}

// ---- scenes (srb_ctx_set_scenes).  A table is in use by a call when the call hands it over: the obstacles with
// n_obs > 0, the neighbour snapshot with a pointer (the metrics: n_all > 0).
// "Up to K nearest" of what exists for an agent: the whole tables, or with scenes its scene's (batch-uniform).
static void clamp_K(const srb_ctx *c, int n_obs, bool has_nbr, int n_all, int *Ko, int *Kn)
{
    int rows = n_obs > 0 ? n_obs : 0, others = has_nbr ? n_all - 1 : 0;
    if (c->scene_agents > 0) {
        rows = std::min(rows, c->scene_obs);
        others = has_nbr ? c->scene_agents - 1 : 0;
    }
    if (*Ko > rows) *Ko = rows;
    if (*Kn > others) *Kn = others > 0 ? others : 0;
}

// The per-call refusals of a scene partition, before anything is launched; *n_scenes (optional) receives the
// number of scenes of the call's tables.  Nothing to check with scenes off, or without a table.
static int check_scenes(const srb_ctx *c, int n_agents, int n_obs, bool has_nbr, int n_all, int agent_offset,
                        int *n_scenes = nullptr)
{
    const int sa = c->scene_agents, so = c->scene_obs;
    if (n_scenes) *n_scenes = 0;
    const bool has_obs = n_obs > 0;
    if (sa <= 0 || (!has_obs && !has_nbr)) return SRB_OK;
    int ns;
    if (has_nbr) {
        if (n_all < 0 || n_all % sa != 0)
            return fail(SRB_ERR_ARG, "scenes: n_all (" + std::to_string(n_all) + ") is not a multiple of scene_agents (" +
                                     std::to_string(sa) + ")");
        ns = n_all / sa;
        if (has_obs && (long long)n_obs != (long long)ns * so)
            return fail(SRB_ERR_ARG, "scenes: n_obs (" + std::to_string(n_obs) + ") != scenes * scene_obs (" +
                                     std::to_string(ns) + " * " + std::to_string(so) + ")");
    } else {
        if (so == 0 || n_obs % so != 0)
            return fail(SRB_ERR_ARG, "scenes: n_obs (" + std::to_string(n_obs) + ") != scenes * scene_obs (scene_obs " +
                                     std::to_string(so) + ")");
        ns = n_obs / so;
    }
    if (agent_offset < 0 || (long long)agent_offset + n_agents > (long long)ns * sa)
        return fail(SRB_ERR_ARG, "scenes: agent_offset + n_agents (" + std::to_string(agent_offset) + " + " +
                                 std::to_string(n_agents) + ") lies beyond the last scene (" + std::to_string(ns) +
                                 " scenes of " + std::to_string(sa) + " agents)");
    if (n_scenes) *n_scenes = ns;
    return SRB_OK;
}

// Obstacle / neighbour selection for a batch (srb_knn_kernel; with a uniform grid per long table,
// srb_grid_build_kernel); shared with the SRB-12 mode (srb12_capi.cpp), which hands over its CoM positions as x0.
static int launch_select(srb_ctx *c, const SrbSelect &q)
{
    const int sel_stride = q.stride();
    hipStream_t s = q.s;
    // scenes: every agent's scene sub-tables brute force, no grid built or consulted (the cached static grid of
    // obstacles_version stays for a later call with scenes off); the plan selection on the scene's rows
    if (c->scene_agents > 0) {
        const bool by_plan = q.nbr_plan && q.K_nbr > 0;
        if (q.K_obs > 0 || !by_plan) {
            hipLaunchKernelGGL(srb_knn_scene_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_WAVES), 0, s, q.n_agents, q.x0,
                               q.obstacles, q.nbr_state, q.agent_offset, c->scene_agents, c->scene_obs, q.K_obs,
                               by_plan ? 0 : q.K_nbr, q.sel, sel_stride);
            HIPCHK(hipGetLastError());
        }
        if (by_plan) {
            hipLaunchKernelGGL(srb_knn_plan_scene_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_PLAN_WAVES), 0, s, q.n_agents,
                               q.x0, q.nbr_state, q.nbr_plan, q.N, q.agent_offset, c->scene_agents, q.K_nbr,
                               q.sel + q.K_obs, sel_stride, q.own_plan);
            HIPCHK(hipGetLastError());
        }
        return SRB_OK;
    }
    // SRB_OPT_PLAN_SELECTION (the caller hands over nbr_plan only then): the neighbour columns by closest predicted
    // approach (srb_knn_plan_kernel, brute force, no grid); the static columns from srb_knn_kernel as ever.
    // own_plan (the SRB-12 mode under a srb_link; else null): the agent's own plan rows, not row g of the table
    if (q.nbr_plan && q.K_nbr > 0) {
        if (q.K_obs > 0)
            if (int rc = launch_select(c, q.obs_only())) return rc;
        hipLaunchKernelGGL(srb_knn_plan_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_PLAN_WAVES), 0, s, q.n_agents, q.x0,
                           q.nbr_state, q.nbr_plan, q.n_all, q.N, q.agent_offset, q.K_nbr, q.sel + q.K_obs, sel_stride,
                           q.own_plan);
        HIPCHK(hipGetLastError());
        return SRB_OK;
    }
    // long tables (a swarm sharded over GPUs: the whole neighbour snapshot, obstacles scaled
    // with the arena) get a uniform grid so each agent scans only the cells around it
    // (a versioned static obstacle table builds its grid once, so it pays off at fewer rows;
    // SRB_OPT_GRID_MIN_ROWS / _STATIC set the thresholds)
    const int min_rows = c->grid_min_rows, min_rows_static = c->grid_min_rows_static;
    const bool go = q.K_obs > 0 && q.n_obs >= (q.obstacles_version != 0 ? min_rows_static : min_rows);
    const bool gn = q.K_nbr > 0 && q.n_all >= min_rows;
    if (go) { int rc = grid_reserve(c, 0, q.n_obs); if (rc) return rc; }
    if (gn) { int rc = grid_reserve(c, 1, q.n_all); if (rc) return rc; }
    const srb_ctx::grid_buf &G0 = c->grid[0], &G1 = c->grid[1];
    // a static obstacle table (same version, pointer and size) keeps its grid
    const bool go_build = go && !(q.obstacles_version != 0 && q.obstacles_version == c->grid_ver &&
                                  q.obstacles == c->grid_src && q.n_obs == c->grid_n);
    if (go_build || gn) {
        hipLaunchKernelGGL(srb_grid_build_kernel, dim3(2), dim3(1024), 0, s,
                           q.obstacles, 2, q.n_obs, go_build ? G0.g : nullptr, G0.off, G0.spos, G0.sidx,
                           q.nbr_state, 4, q.n_all, gn ? G1.g : nullptr, G1.off, G1.spos, G1.sidx);
        HIPCHK(hipGetLastError());
    }
    if (go_build) { c->grid_src = q.obstacles; c->grid_n = q.n_obs; c->grid_ver = q.obstacles_version; }
    hipLaunchKernelGGL(srb_knn_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_WAVES), 0, s, q.n_agents, q.x0, q.obstacles,
                       q.n_obs, q.nbr_state, q.n_all, q.agent_offset, q.K_obs, q.K_nbr, q.sel, sel_stride,
                       go ? G0.g : nullptr, G0.off, G0.spos, G0.sidx,
                       gn ? G1.g : nullptr, G1.off, G1.spos, G1.sidx);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// The horizon-aware obstacle selection (srb_moving.horizon_selection; srb_moving.hip) into the static columns
// 0 .. K_obs - 1 of sel: brute force, with scenes over the agent's scene.  q.N, q.Ts: the grid of the horizon (the
// SRB-12 mode hands over its own).
static int launch_obs_horizon(srb_ctx *c, const SrbSelect &q)
{
    if (c->scene_agents > 0)
        hipLaunchKernelGGL(srb_knn_obs_horizon_scene_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_OBS_WAVES), 0, q.s,
                           q.n_agents, q.x0, q.obstacles, q.t.obs_vel, q.N, q.Ts, q.agent_offset, c->scene_agents,
                           c->scene_obs, q.K_obs, q.sel, q.stride());
    else
        hipLaunchKernelGGL(srb_knn_obs_horizon_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_OBS_WAVES), 0, q.s, q.n_agents,
                           q.x0, q.obstacles, q.t.obs_vel, q.n_obs, q.N, q.Ts, q.K_obs, q.sel, q.stride());
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// The clearance selection (srb_sizes.clearance_selection; srb_sizes.hip) into the static columns 0 .. K_obs - 1 of sel:
// launch_obs_horizon's geometry.  Without the horizon flag the key's distance is the one now (the kernel gets no
// velocities); with it the horizon's minimum.
static int launch_obs_clear(srb_ctx *c, const SrbSelect &q)
{
    const double *obs_vel = q.t.obs_horizon ? q.t.obs_vel : nullptr;
    if (c->scene_agents > 0)
        hipLaunchKernelGGL(srb_knn_obs_clear_scene_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_OBS_WAVES), 0, q.s,
                           q.n_agents, q.x0, q.obstacles, obs_vel, q.t.obs_eps, q.N, q.Ts, q.agent_offset, c->scene_agents,
                           c->scene_obs, q.K_obs, q.sel, q.stride());
    else
        hipLaunchKernelGGL(srb_knn_obs_clear_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_OBS_WAVES), 0, q.s, q.n_agents,
                           q.x0, q.obstacles, obs_vel, q.t.obs_eps, q.n_obs, q.N, q.Ts, q.K_obs, q.sel, q.stride());
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// The neighbour clearance selection (srb_agent_sizes.clearance_selection; srb_agents.hip) of a neighbour-only request
// (SrbSelect::nbr_only: q.sel points at the neighbour columns): brute force, with scenes over the agent's scene.
// q.nbr_plan null: the key's distance is the snapshot's; else the horizon's minimum.
static int launch_nbr_clear(srb_ctx *c, const SrbSelect &q)
{
    if (c->scene_agents > 0)
        hipLaunchKernelGGL(srb_knn_nbr_clear_scene_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_PLAN_WAVES), 0, q.s,
                           q.n_agents, q.x0, q.nbr_state, q.nbr_plan, q.t.agent_rad, q.N, q.agent_offset, c->scene_agents,
                           q.K_nbr, q.sel, q.stride());
    else
        hipLaunchKernelGGL(srb_knn_nbr_clear_kernel, dim3(q.n_agents), dim3(64 * SRB_KNN_PLAN_WAVES), 0, q.s, q.n_agents,
                           q.x0, q.nbr_state, q.nbr_plan, q.t.agent_rad, q.n_all, q.N, q.agent_offset, q.K_nbr, q.sel,
                           q.stride());
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// The columns of one side by what q asks for them.  Static: with srb_sizes' flag by clearance to the level set (over
// the horizon when srb_moving's flag is set too, else now), with srb_moving's flag alone by closest predicted
// approach over the grid (q.N, q.Ts), else by centres.  Neighbours: with srb_agent_sizes' flag by clearance (over the
// horizon with q.nbr_plan, else now), else launch_select's (by q.nbr_plan or the snapshot).
static int select_obs(srb_ctx *c, const SrbSelect &q)
{
    if (q.K_obs == 0) return SRB_OK;
    if (q.t.obs_clear) return launch_obs_clear(c, q);
    if (q.t.obs_horizon) return launch_obs_horizon(c, q);
    return launch_select(c, q.obs_only());
}

static int select_nbr(srb_ctx *c, const SrbSelect &q)
{
    if (q.K_nbr == 0) return SRB_OK;
    return q.t.nbr_clear ? launch_nbr_clear(c, q.nbr_only()) : launch_select(c, q.nbr_only());
}

// The selection of a solve, both modes: with any flag of q.t the two sides one after the other, without one the one
// launch of launch_select.  q.own_plan (srb12_solve_batch_link_device): the caller refuses it together with nbr_clear
int srb_internal_select(srb_ctx *c, const SrbSelect &q)
{
    if (!q.t.obs_clear && !q.t.obs_horizon && !q.t.nbr_clear) return launch_select(c, q);
    if (int rc = select_nbr(c, q)) return rc;
    return select_obs(c, q);
}

int srb_internal_mark_done(srb_ctx *c, hipStream_t s) { return c->order.mark_done(s); }

int srb_internal_check_scenes(const srb_ctx *c, int n_agents, int n_obs, bool has_nbr, int n_all, int agent_offset)
{
    return check_scenes(c, n_agents, n_obs, has_nbr, n_all, agent_offset);
}

void srb_internal_clamp_K(const srb_ctx *c, int n_obs, bool has_nbr, int n_all, int *Ko, int *Kn)
{
    clamp_K(c, n_obs, has_nbr, n_all, Ko, Kn);
}

// the checks of srb_moving, srb_sizes and srb_agent_sizes that need no context (srb_host.h), with this mode's names in
// the messages
static int check_tables(const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, const srb_batch *b,
                        bool rollout)
{
    return srb_check_tables(mv, sz, ag, b, rollout, "srb_rollout_moving_device", "srb_batch");
}

// The argument errors of the plan members (srb_batch.nbr_plan / plan), before anything is launched.  select: the
// call would run the neighbour selection (the horizon-aware one then needs the table).
static int check_plans(srb_ctx *c, int n_agents, const srb_batch *d, bool select)
{
    const srb_params *p = &c->p;
    if (d->nbr_plan && !d->nbr_state) return fail(SRB_ERR_ARG, "nbr_plan needs nbr_state (the selection's snapshot)");
    if (d->nbr_plan && p->K_nbr > 0 && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return fail(SRB_ERR_ARG, "nbr_plan: agent_offset + n_agents exceeds n_all (the plan table's rows)");
    if (srb_overlap(d->plan, (size_t)n_agents * 2 * p->N, d->nbr_plan, (size_t)std::max(d->n_all, 0) * 2 * p->N))
        return fail(SRB_ERR_ARG, "plan overlaps the nbr_plan table (workgroups read the table while others write their "
                                 "plans: use two buffers)");
    if (select && c->plan_selection && !d->nbr_plan && d->nbr_state && std::min(p->K_nbr, d->n_all - 1) > 0)
        return fail(SRB_ERR_ARG, "SRB_OPT_PLAN_SELECTION = 1 needs nbr_plan (the horizon-aware selection reads the plan table)");
    return SRB_OK;
}

// t: the tables of srb_moving, srb_sizes and srb_agent_sizes (SrbTables{}: none, every launch as without them)
static int launch(srb_ctx *c, int n_agents, const srb_batch *d, hipStream_t s, int use_nlp, const SrbTables &t)
{
    if (n_agents < 0 || n_agents > c->max_agents) return fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    const srb_params *p = &c->p;
    if (!d->x0 || !d->ref || !d->foot || !d->x || !d->obj || !d->status || !d->iters)
        return fail(SRB_ERR_ARG, "missing buffer");
    if ((d->alpha != nullptr) != (d->alpha_buf != nullptr))
        return fail(SRB_ERR_ARG, "alpha and alpha_buf go together (both or neither)");
    if (d->alpha && p->N < 4) return fail(SRB_ERR_ARG, "the Bezier fit needs N >= 4 (X_0..X_3)");
    if (int rc = check_scenes(c, n_agents, d->n_obs, d->nbr_state != nullptr, d->n_all, d->agent_offset)) return rc;
    if (use_nlp && p->K_obs > 0 && (d->n_obs < 0 || (d->n_obs > 0 && !d->obstacles)))
        return fail(SRB_ERR_ARG, "obstacles missing");
    if (use_nlp && p->K_nbr > 0 && d->nbr_state && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return fail(SRB_ERR_ARG, "agent_offset out of range of the neighbour table");
    if (use_nlp && (t.agent_rad || t.agent_pad) && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return fail(SRB_ERR_ARG, "srb_agent_sizes: agent_offset + n_agents exceeds n_all (the agent tables' rows)");
    // (the QP-only solve ignores nbr_plan: it has no obstacle rows)
    if (use_nlp)
        if (int rc = check_plans(c, n_agents, d, c->selection != 0)) return rc;
    const double *nbr_plan = (use_nlp && p->K_nbr > 0) ? d->nbr_plan : nullptr;
    SrbKParams k = make_kparams(p, use_nlp);
    k.qp_init = c->qp_init;
    k.polish_rho = c->polish_rho;
    k.qp_warm_tol = c->qp_warm_tol;
    k.kkt32_mu = c->kkt32_mu;
    k.kkt32_ref = c->kkt32_ref;
    // "up to K nearest": clamp to what exists (batch-uniform), so no row is ever a dummy
    // (with scenes: to the agent's scene)
    clamp_K(c, d->n_obs, d->nbr_state != nullptr, d->n_all, &k.K_obs, &k.K_nbr);
    const srb_instance *in = pick_instance(k, wanted_waves(n_agents, srb_slots(k.N, k.C, k.K_obs + k.K_nbr), c->nw));
    if (!in) return fail(SRB_ERR_SIZE, "no kernel instance covers this problem");
    const size_t lds = (size_t)srb_lds_doubles(k, in->nzl, in->nw) * sizeof(double);
    c->last_nw = in->nw;
    HIPCHK(hipSetDevice(c->device));
    const int n_obs = k.K_obs > 0 ? d->n_obs : 0, n_all = k.K_nbr > 0 ? d->n_all : 0;
    // timing events (SRB_OPT_TIMING): each record is a marker the queue drains to, a few us a step
    c->timed = c->timing != 0;
    if (c->timing) HIPCHK(hipEventRecord(c->ev[0], s));
    // two launches: nearest obstacle / neighbour selection, then QP and NLP stages per agent
    int *sel = d->sel ? d->sel : c->sel;
    // SRB_OPT_SELECTION 0: the caller filled d->sel by srb_select_device (its two tables may then be selected
    // around a collective, bench.py's multi-GPU step)
    // (with srb_moving.horizon_selection the static columns by closest predicted approach: srb_internal_select)
    if (use_nlp && k.K_obs + k.K_nbr > 0 && c->selection) {
        SrbSelect q = {};
        q.n_agents = n_agents; q.x0 = d->x0; q.agent_offset = d->agent_offset;
        q.obstacles = d->obstacles; q.n_obs = n_obs; q.obstacles_version = d->obstacles_version;
        q.nbr_state = d->nbr_state; q.n_all = n_all;
        q.K_obs = k.K_obs; q.K_nbr = k.K_nbr; q.sel = sel; q.s = s;
        q.N = k.N; q.Ts = p->Ts;
        q.nbr_plan = c->plan_selection ? nbr_plan : nullptr;
        q.t = t;
        if (int rc = srb_internal_select(c, q)) return rc;
    }
    // (the QP-only solve reads no table)
    const SrbTables g = t.gated(use_nlp && k.K_obs > 0, use_nlp && k.K_nbr > 0);
    const double *vel = g.obs_vel, *eps = g.obs_eps, *rad = g.agent_rad, *pad = g.agent_pad;
    const bool tabled = g.any_solve_table();
    if (c->timing) HIPCHK(hipEventRecord(c->ev[2], s));
    // the solve kernel, then (NLP stage) the active-set polish of its result: fused into the solve
    // kernel's end (SRB_OPT_POLISH_FUSED, instances up to SRB_FUSED_POLISH_MAX = NZL 24), else srb_polish_kernel (same instance
    // geometry; it rewrites x / obj / alpha / status only where the polish is accepted)
    const bool fused = use_nlp && c->polish && c->polish_fused && SRB_FUSED_POLISH_OK(in->nzl);
    const bool polish = use_nlp && c->polish && !fused;
    k.polish_fused = fused ? 1 : 0;
    c->last_polish = fused ? 2 : polish ? 1 : 0;
    // SRB_OPT_KKT_FP32_MU > 0: the instance's fp32-factor variant where one is compiled (else the fp64 one)
    srb_kernel_fn fn = in->fn;
    srb_kernel_mv_fn fn_mv = in->fn_mv;
    const char *fn_name = in->fn_name, *fn_mv_name = in->fn_mv_name;
    c->last_f32 = 0;
    if (c->kkt32_mu > 0.0) {
        const srb_instance *f = f32_variant(in);
        if (f) { fn = f->fn; fn_mv = f->fn_mv; fn_name = f->fn_name; fn_mv_name = f->fn_mv_name; c->last_f32 = 1; }
    }
    c->last_solve_name = tabled ? fn_mv_name : fn_name;      // what the launch below runs (srb_ctx_last_kernels)
    c->last_polish_name = "";
    // with any of the four tables the instance's table kernels (further arguments); without, the launches as ever
    if (tabled)
        hipLaunchKernelGGL(fn_mv, dim3(n_agents), dim3(64 * in->nw), lds, s, k, n_agents, d->x0, d->ref, d->foot, d->obstacles,
                           n_obs, d->nbr_state, n_all, d->agent_offset, d->x_qp, d->x, d->obj, d->status, d->iters,
                           d->alpha ? d->alpha_buf : nullptr, d->alpha_buf ? d->alpha : nullptr, (const int *)sel,
                           polish ? c->zpol : nullptr, c->zstride, k.K_nbr > 0 ? nbr_plan : nullptr, d->plan, vel, eps,
                           rad, pad);
    else
        hipLaunchKernelGGL(fn, dim3(n_agents), dim3(64 * in->nw), lds, s, k, n_agents, d->x0, d->ref, d->foot, d->obstacles,
                           n_obs, d->nbr_state, n_all, d->agent_offset, d->x_qp, d->x, d->obj, d->status, d->iters,
                           d->alpha ? d->alpha_buf : nullptr, d->alpha_buf ? d->alpha : nullptr, (const int *)sel,
                           polish ? c->zpol : nullptr, c->zstride, k.K_nbr > 0 ? nbr_plan : nullptr, d->plan);
    HIPCHK(hipGetLastError());
    if (c->timing) HIPCHK(hipEventRecord(c->ev[3], s));
    if (polish) {
        // the polish kernel reads only the solve's outputs (x, status, sel, zpol by global slot
        // index), so it runs at its own waves per agent: at least two (its registers fit two
        // waves per SIMD, and a polish step's latency halves): configs[2] polish 0.067 -> 0.053 ms,
        // configs[1] (solve at 4 waves) and N = 20 (2 waves) unchanged, one wave slower everywhere
        // (profiles/r03_polish_nw_ab.txt).  SRB_OPT_POLISH_WAVES = 1 | 2 | 4 overrides.
        const int pnw = c->polish_waves ? c->polish_waves : (in->nw < 2 ? 2 : in->nw);
        const srb_instance *pin = pnw == in->nw ? in : pick_instance(k, pnw);
        if (!pin || pin->nzl != in->nzl) pin = in;
        const size_t plds = (size_t)srb_lds_doubles(k, pin->nzl, pin->nw) * sizeof(double);
        c->last_polish_name = tabled ? pin->polish_mv_name : pin->polish_name;
        if (tabled)
            hipLaunchKernelGGL(pin->polish_mv, dim3(n_agents), dim3(64 * pin->nw), plds, s, k, n_agents, d->x0, d->ref, d->foot,
                               d->obstacles, d->nbr_state, d->x, d->obj, d->status, d->alpha ? d->alpha_buf : nullptr,
                               d->alpha_buf ? d->alpha : nullptr, (const int *)sel, (const float *)c->zpol, c->zstride,
                               k.K_nbr > 0 ? nbr_plan : nullptr, d->plan, vel, eps, rad, pad, d->agent_offset);
        else
            hipLaunchKernelGGL(pin->polish, dim3(n_agents), dim3(64 * pin->nw), plds, s, k, n_agents, d->x0, d->ref, d->foot,
                               d->obstacles, d->nbr_state, d->x, d->obj, d->status, d->alpha ? d->alpha_buf : nullptr,
                               d->alpha_buf ? d->alpha : nullptr, (const int *)sel, (const float *)c->zpol, c->zstride,
                               k.K_nbr > 0 ? nbr_plan : nullptr, d->plan);
        HIPCHK(hipGetLastError());
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev[1], s));
    return SRB_OK;
}

extern "C" int srb_ctx_set_waves(srb_ctx *c, int nw)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (nw != 0 && nw != 1 && nw != 2 && nw != 4) return fail(SRB_ERR_ARG, "waves per agent: 0 (automatic), 1, 2 or 4");
    c->nw = nw;
    return SRB_OK;
}

extern "C" int srb_ctx_waves(srb_ctx *c) { return c ? c->last_nw : 0; }

extern "C" int srb_ctx_last_kernels(srb_ctx *c, const char **solve, const char **polish)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (solve) *solve = c->last_solve_name;
    if (polish) *polish = c->last_polish_name;
    return SRB_OK;
}

// the instance table and the pick, host only (no HIP call: usable without a device)
extern "C" int srb_kernel_table(int i, int dims[6], const char **name)
{
    const int n64 = (int)(sizeof g_instances / sizeof g_instances[0]), n32 = (int)(sizeof g_instances_f32 / sizeof g_instances_f32[0]);
    if (i < 0 || i >= n64 + n32) return fail(SRB_ERR_ARG, "srb_kernel_table: index past the end");
    const srb_instance &in = i < n64 ? g_instances[i] : g_instances_f32[i - n64];
    if (dims) { dims[0] = in.nzl; dims[1] = in.ts; dims[2] = in.nw; dims[3] = in.nc; dims[4] = in.cc; dims[5] = in.kc; }
    if (name) *name = in.fn_name;
    return SRB_OK;
}

extern "C" int srb_pick_kernel(const srb_params *p, int waves, int dims[6])
{
    if (!p || !dims) return fail(SRB_ERR_ARG, "srb_pick_kernel: null argument");
    if (waves != 1 && waves != 2 && waves != 4) return fail(SRB_ERR_ARG, "waves per agent: 1, 2 or 4");
    const SrbKParams k = make_kparams(p, p->use_nlp);
    const srb_instance *in = pick_instance(k, waves, (size_t)160 * 1024);
    if (!in) return fail(SRB_ERR_SIZE, "no kernel instance covers this problem");
    dims[0] = in->nzl; dims[1] = in->ts; dims[2] = in->nw; dims[3] = in->nc; dims[4] = in->cc; dims[5] = in->kc;
    return SRB_OK;
}

extern "C" int srb_ctx_set_scenes(srb_ctx *c, int scene_agents, int scene_obs)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (scene_agents < 0 || scene_obs < 0) return fail(SRB_ERR_ARG, "scenes: scene_agents and scene_obs must not be negative");
    if (scene_agents == 0 && scene_obs != 0)
        return fail(SRB_ERR_ARG, "scenes: scene_agents == 0 (off) goes with scene_obs == 0");
    c->scene_agents = scene_agents;
    c->scene_obs = scene_obs;
    return SRB_OK;
}

extern "C" int srb_ctx_scenes(srb_ctx *c, int *scene_agents, int *scene_obs)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (scene_agents) *scene_agents = c->scene_agents;
    if (scene_obs) *scene_obs = c->scene_obs;
    return SRB_OK;
}

extern "C" int srb_ctx_set_option(srb_ctx *c, int opt, double v)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    const bool whole = v == (double)(long long)v;
    switch (opt) {
    case SRB_OPT_POLISH:
        if (v != 0.0 && v != 1.0) return fail(SRB_ERR_ARG, "SRB_OPT_POLISH: 0 or 1");
        c->polish = (int)v; return SRB_OK;
    case SRB_OPT_POLISH_RHO:
        if (!(v >= 1e3 && v <= 1e12)) return fail(SRB_ERR_ARG, "SRB_OPT_POLISH_RHO: 1e3 .. 1e12");
        c->polish_rho = v; return SRB_OK;
    case SRB_OPT_POLISH_WAVES:
        if (v != 0.0 && v != 1.0 && v != 2.0 && v != 4.0) return fail(SRB_ERR_ARG, "SRB_OPT_POLISH_WAVES: 0 (automatic), 1, 2 or 4");
        c->polish_waves = (int)v; return SRB_OK;
    case SRB_OPT_POLISH_FUSED:
        if (v != 0.0 && v != 1.0) return fail(SRB_ERR_ARG, "SRB_OPT_POLISH_FUSED: 0 or 1");
        c->polish_fused = (int)v; return SRB_OK;
    case SRB_OPT_LAST_POLISH:
        return fail(SRB_ERR_ARG, "SRB_OPT_LAST_POLISH is read only");
    case SRB_OPT_QP_WARM_TOL:
        if (!(v >= 0.0 && v <= 1e3)) return fail(SRB_ERR_ARG, "SRB_OPT_QP_WARM_TOL: 0 (the full tolerance) .. 1e3");
        c->qp_warm_tol = v; return SRB_OK;
    case SRB_OPT_TIMING:
        if (v != 0.0 && v != 1.0) return fail(SRB_ERR_ARG, "SRB_OPT_TIMING: 0 or 1");
        c->timing = (int)v; return SRB_OK;
    case SRB_OPT_SELECTION:
        if (v != 0.0 && v != 1.0) return fail(SRB_ERR_ARG, "SRB_OPT_SELECTION: 0 or 1");
        c->selection = (int)v; return SRB_OK;
    case SRB_OPT_KKT_FP32_MU:
        if (!(v >= 0.0 && v <= 1e30)) return fail(SRB_ERR_ARG, "SRB_OPT_KKT_FP32_MU: 0 (off) .. 1e30");
        c->kkt32_mu = v; return SRB_OK;
    case SRB_OPT_KKT_FP32_REFINE:
        if (!whole || v < 1.0 || v > 8.0) return fail(SRB_ERR_ARG, "SRB_OPT_KKT_FP32_REFINE: 1 .. 8");
        c->kkt32_ref = (int)v; return SRB_OK;
    case SRB_OPT_LAST_KKT_FP32:
        return fail(SRB_ERR_ARG, "SRB_OPT_LAST_KKT_FP32 is read only");
    case SRB_OPT_PLAN_SELECTION:
        if (v != 0.0 && v != 1.0) return fail(SRB_ERR_ARG, "SRB_OPT_PLAN_SELECTION: 0 (snapshot) or 1 (closest predicted approach)");
        c->plan_selection = (int)v; return SRB_OK;
    case SRB_OPT_GRID_MIN_ROWS:
    case SRB_OPT_GRID_MIN_ROWS_STATIC:
        if (!whole || v < 1.0 || v > 2147483647.0) return fail(SRB_ERR_ARG, "SRB_OPT_GRID_MIN_ROWS*: a row count >= 1");
        (opt == SRB_OPT_GRID_MIN_ROWS ? c->grid_min_rows : c->grid_min_rows_static) = (int)v;
        return SRB_OK;
    default:
        return fail(SRB_ERR_ARG, "unknown option");
    }
}

extern "C" int srb_ctx_get_option(srb_ctx *c, int opt, double *v)
{
    if (!c || !v) return fail(SRB_ERR_ARG, "null argument");
    switch (opt) {
    case SRB_OPT_POLISH: *v = c->polish; return SRB_OK;
    case SRB_OPT_POLISH_RHO: *v = c->polish_rho; return SRB_OK;
    case SRB_OPT_POLISH_WAVES: *v = c->polish_waves; return SRB_OK;
    case SRB_OPT_GRID_MIN_ROWS: *v = c->grid_min_rows; return SRB_OK;
    case SRB_OPT_GRID_MIN_ROWS_STATIC: *v = c->grid_min_rows_static; return SRB_OK;
    case SRB_OPT_POLISH_FUSED: *v = c->polish_fused; return SRB_OK;
    case SRB_OPT_LAST_POLISH: *v = c->last_polish; return SRB_OK;
    case SRB_OPT_TIMING: *v = c->timing; return SRB_OK;
    case SRB_OPT_QP_WARM_TOL: *v = c->qp_warm_tol; return SRB_OK;
    case SRB_OPT_SELECTION: *v = c->selection; return SRB_OK;
    case SRB_OPT_KKT_FP32_MU: *v = c->kkt32_mu; return SRB_OK;
    case SRB_OPT_KKT_FP32_REFINE: *v = c->kkt32_ref; return SRB_OK;
    case SRB_OPT_LAST_KKT_FP32: *v = c->last_f32; return SRB_OK;
    case SRB_OPT_PLAN_SELECTION: *v = c->plan_selection; return SRB_OK;
    default: return fail(SRB_ERR_ARG, "unknown option");
    }
}

extern "C" int srb_ctx_set_qp_init(srb_ctx *c, int mode)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (mode != 0 && mode != 1) return fail(SRB_ERR_ARG, "QP start: 1 (scaled, default) or 0 (iSWIFT kkt_initialize)");
    c->qp_init = mode;
    return SRB_OK;
}

// (the plain, the _moving and the _sized entry points are this one without a table: one path)
extern "C" int srb_solve_batch_agents_device(srb_ctx *c, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                                             const srb_sizes *sz, const srb_agent_sizes *ag, void *stream)
{
    if (int rc0 = srb_check_struct(dev_io, "srb_batch")) return rc0;   // first: it needs no context
    if (int rc0 = check_tables(mv, sz, ag, dev_io, false)) return rc0;
    if (!c || !dev_io) return fail(SRB_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;          // NULL: the HIP null stream (ordered with blocking streams)
    HIPCHK(hipSetDevice(c->device));
    int rc = c->order.order_after_last(s);
    if (!rc) rc = launch(c, n_agents, dev_io, s, c->p.use_nlp, srb_tables(mv, sz, ag));
    if (!rc && n_agents > 0) rc = c->order.mark_done(s);
    return rc;
}

extern "C" int srb_solve_batch_sized_device(srb_ctx *c, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                                            const srb_sizes *sz, void *stream)
{
    return srb_solve_batch_agents_device(c, n_agents, dev_io, mv, sz, nullptr, stream);
}

extern "C" int srb_solve_batch_device(srb_ctx *c, int n_agents, const srb_batch *dev_io, void *stream)
{
    return srb_solve_batch_sized_device(c, n_agents, dev_io, nullptr, nullptr, stream);
}

extern "C" int srb_solve_batch_moving_device(srb_ctx *c, int n_agents, const srb_batch *dev_io, const srb_moving *mv,
                                             void *stream)
{
    return srb_solve_batch_sized_device(c, n_agents, dev_io, mv, nullptr, stream);
}

// One or both tables of the selection into d->sel (required; [A][Ko + Kn], the layout the solve reads):
// tables bit 0 the static obstacles (its columns 0 .. Ko - 1), bit 1 the neighbour snapshot (Ko .. Ko + Kn - 1).
// With SRB_OPT_SELECTION = 0 the solve then uses sel as it is, so a caller can select the static obstacles
// while the neighbour all-gather is in flight and the neighbours after it (bench.py).
// A flag of mv, sz or ag chooses the launcher of its side, as in the solve's own selection (select_obs, select_nbr:
// srb_moving.horizon_selection, srb_sizes.clearance_selection for tables & 1, srb_agent_sizes.clearance_selection for
// tables & 2); an entry point whose struct or flag is absent is the one below it, since the snapshot selection reads
// no table.
extern "C" int srb_select_agents_device(srb_ctx *c, int n_agents, const srb_batch *d, const srb_moving *mv,
                                        const srb_sizes *sz, const srb_agent_sizes *ag, int tables, void *stream)
{
    if (int rc0 = srb_check_struct(d, "srb_batch")) return rc0;
    if (int rc0 = check_tables(mv, sz, ag, d, false)) return rc0;
    if (!c || !d) return fail(SRB_ERR_ARG, "null argument");
    if (tables < 1 || tables > 3) return fail(SRB_ERR_ARG, "tables: 1 (static obstacles), 2 (neighbours) or 3 (both)");
    if (n_agents < 0 || n_agents > c->max_agents) return fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (!d->x0 || !d->sel) return fail(SRB_ERR_ARG, "missing buffer (x0, sel)");
    if (n_agents == 0) return SRB_OK;
    int Ko = c->p.K_obs, Kn = c->p.K_nbr;                 // clamped exactly as the solve does
    clamp_K(c, d->n_obs, d->nbr_state != nullptr, d->n_all, &Ko, &Kn);
    if (int rc0 = check_scenes(c, n_agents, d->n_obs, d->nbr_state != nullptr, d->n_all, d->agent_offset)) return rc0;
    SrbSelect q = {};
    q.n_agents = n_agents; q.x0 = d->x0; q.agent_offset = d->agent_offset;
    q.obstacles = d->obstacles; q.n_obs = Ko > 0 ? d->n_obs : 0; q.obstacles_version = d->obstacles_version;
    q.nbr_state = d->nbr_state; q.n_all = Kn > 0 ? d->n_all : 0;
    q.K_obs = Ko; q.K_nbr = Kn; q.sel = d->sel; q.s = (hipStream_t)stream;
    q.N = c->p.N; q.Ts = c->p.Ts;
    q.nbr_plan = (c->plan_selection && (tables & 2)) ? d->nbr_plan : nullptr;
    q.t = srb_tables(mv, sz, ag);
    // only the flags of the sides that this call selects count
    if (!(tables & 1)) q.t.obs_horizon = q.t.obs_clear = 0;
    if (!(tables & 2)) q.t.nbr_clear = 0;
    const bool obs_flag = q.t.obs_horizon || q.t.obs_clear, nbr_flag = q.t.nbr_clear != 0;
    // The refusals of the two sides, in the order they have always had: the neighbour side's first where its flag
    // is set; and a call for the static columns alone under their flag never looked at the plan members.
    const bool no_obstacles = (tables & 1) && Ko > 0 && !d->obstacles;
    if (no_obstacles && !nbr_flag) return fail(SRB_ERR_ARG, "obstacles missing");
    if ((tables & 2) && Kn > 0 && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return fail(SRB_ERR_ARG, "agent_offset out of range of the neighbour table");
    if ((tables & 2) || !obs_flag)
        if (int rc0 = check_plans(c, n_agents, d, (tables & 2) != 0)) return rc0;
    if (no_obstacles) return fail(SRB_ERR_ARG, "obstacles missing");
    // Without a flag one launch serves both sides; with one, a launch per side (the flagged side last, the neighbour
    // side's flag before the static side's)
    return c->order.run(c->device, q.s, [&] {
        int rc = SRB_OK;
        if (nbr_flag) {
            if (tables & 1) rc = select_obs(c, q);
            return rc ? rc : select_nbr(c, q);
        }
        if (obs_flag) {
            if (tables & 2) rc = select_nbr(c, q);
            return rc ? rc : select_obs(c, q);
        }
        return tables == 1 ? select_obs(c, q) : tables == 2 ? select_nbr(c, q) : Ko + Kn > 0 ? launch_select(c, q) : rc;
    });
}

// (the _sized, the _moving and the plain entry points are the _agents one without a table: one path)
extern "C" int srb_select_sized_device(srb_ctx *c, int n_agents, const srb_batch *d, const srb_moving *mv,
                                       const srb_sizes *sz, int tables, void *stream)
{
    return srb_select_agents_device(c, n_agents, d, mv, sz, nullptr, tables, stream);
}

extern "C" int srb_select_moving_device(srb_ctx *c, int n_agents, const srb_batch *d, const srb_moving *mv, int tables,
                                        void *stream)
{
    return srb_select_sized_device(c, n_agents, d, mv, nullptr, tables, stream);
}

extern "C" int srb_select_device(srb_ctx *c, int n_agents, const srb_batch *d, int tables, void *stream)
{
    return srb_select_sized_device(c, n_agents, d, nullptr, nullptr, tables, stream);
}

extern "C" int srb_obstacles_advance_device(srb_ctx *c, int n_obs, double *obstacles, const double *obs_vel, void *stream)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    if (n_obs < 0) return fail(SRB_ERR_ARG, "srb_obstacles_advance_device: negative n_obs");
    if (n_obs == 0) return SRB_OK;
    if (!obstacles || !obs_vel) return fail(SRB_ERR_ARG, "srb_obstacles_advance_device: obstacles / obs_vel missing");
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] { return srb_launch_obstacles_advance(n_obs, c->p.Ts, obstacles, obs_vel, s); });
}

extern "C" int srb_prepare_batch_device(srb_ctx *c, int n_agents, const srb_prep *d, void *stream)
{
    if (int rc0 = srb_check_struct(d, "srb_prep")) return rc0;     // first: it needs no context
    if (!c || !d) return fail(SRB_ERR_ARG, "null argument");
    if (n_agents < 0) return fail(SRB_ERR_ARG, "negative n_agents");
    if (n_agents == 0) return SRB_OK;
    if (!d->Pr || !d->Prd || !d->gait_domain || !d->contact || !d->toe || !d->start || !d->q || !d->dq || !d->x0 ||
        !d->ref || !d->foot || !d->last_state || !d->status)
        return fail(SRB_ERR_ARG, "missing buffer");
    if (d->n_rows < 2 || d->T < 1) return fail(SRB_ERR_ARG, "empty HL path");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;          // NULL: the HIP null stream (ordered with blocking streams)
    hipLaunchKernelGGL(srb_prepare_kernel, dim3((n_agents + 255) / 256), dim3(256), 0, s, n_agents, c->p.N, c->p.C,
                       d->n_rows, d->T, d->agent_offset, d->Pr, d->Prd, d->agent_id, d->gait_domain, d->contact,
                       d->toe, d->start, d->q, d->dq, d->x0, d->ref, d->foot, d->last_state, d->status);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// ---- closed-loop rollout (srb_sim.hip): the argument checks that need no context come first, in a fixed order
// (struct_size, goal, x), so that tests/test_rollout.py reaches them without a GPU
static int check_sim(const srb_sim *d, int cycle, bool advance)
{
    if (int rc = srb_check_struct(d, "srb_sim")) return rc;
    if (!d) return fail(SRB_ERR_ARG, "null argument");
    if (cycle < d->c_first) return fail(SRB_ERR_ARG, "srb_sim: cycle precedes c_first");
    if (!advance) return SRB_OK;
    if (!d->goal) return fail(SRB_ERR_ARG, "srb_sim.goal missing");
    if (!d->x && cycle != d->c_first)
        return fail(SRB_ERR_ARG, "srb_sim.x missing (the previous solve's x: required when cycle != c_first)");
    return SRB_OK;
}

// The argument errors of srb_plant that need no context, before anything is launched.  has_x: the call has the
// previous solve's x (srb_sim.x for the advance; the rollout wires batch.x in and reports that itself).
#define SRB_PLANT_MAX_PUSH 4096
static int check_plant(const srb_plant *pl, bool has_x)
{
    if (int rc = srb_check_struct(pl, "srb_plant")) return rc;
    if (!pl) return SRB_OK;
    if (pl->n_push < 0 || pl->n_push > SRB_PLANT_MAX_PUSH)
        return fail(SRB_ERR_ARG, "srb_plant.n_push: 0 .. 4096 (every agent scans the whole push table)");
    if (pl->n_push > 0 && (!pl->push_cycle || !pl->push_agent || !pl->push_dv))
        return fail(SRB_ERR_ARG, "srb_plant.n_push > 0 needs push_cycle, push_agent and push_dv");
    if (pl->plant_hcom && !has_x)
        return fail(SRB_ERR_ARG, "srb_plant.plant_hcom needs srb_sim.x (the plant is driven by the inputs the model applied)");
    return SRB_OK;
}

// the struct disturbs the plant at all (else every entry point is the one it extends; dist_log alone is not written)
static bool plant_on(const srb_plant *pl) { return pl && (pl->kick_v || pl->kick_p || pl->plant_hcom || pl->n_push > 0); }

// pl: the disturbed plant (null: nominal).  It acts from the second cycle on; at c_first the state is the caller's.
static int launch_advance(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, hipStream_t s,
                          const srb_plant *pl = nullptr)
{
    const srb_params *p = &c->p;
    if (p->N < 4) return fail(SRB_ERR_ARG, "the rollout needs N >= 4 (one cycle is one gait domain of 4 grids)");
    if (!d->state || !d->x0 || !d->ref || !d->foot || !d->last_state)
        return fail(SRB_ERR_ARG, "srb_sim: missing buffer (state, x0, ref, foot, last_state)");
    if (pl && cycle != d->c_first) {
        const int n_all = d->n_all > 0 ? d->n_all : n_agents;
        if (d->agent_offset < 0 || d->agent_offset + n_agents > n_all)
            return fail(SRB_ERR_ARG, "srb_plant: agent_offset + n_agents exceeds n_all (the plant tables' rows)");
        hipLaunchKernelGGL(srb_sim_advance_plant_kernel, dim3((n_agents + 255) / 256), dim3(256), 0, s, n_agents, p->N,
                           p->C, srb_nv(p), p->Ts, d->vref, cycle, d->c_first, d->state, d->goal, d->phase, d->x,
                           d->status, d->iters, d->x0, d->ref, d->foot, d->last_state, d->alpha_buf, d->plan_table,
                           d->traj, d->status_log, d->iters_log, d->x_log, d->agent_offset, p->grav,
                           (unsigned)(pl->seed & 0xffffffffull), (unsigned)(pl->seed >> 32), pl->kick_v, pl->kick_p,
                           pl->plant_hcom, pl->n_push, pl->push_cycle, pl->push_agent, pl->push_dv, pl->dist_log);
        HIPCHK(hipGetLastError());
        return SRB_OK;
    }
    hipLaunchKernelGGL(srb_sim_advance_kernel, dim3((n_agents + 255) / 256), dim3(256), 0, s, n_agents, p->N, p->C,
                       srb_nv(p), p->Ts, d->vref, cycle, d->c_first, d->state, d->goal, d->phase, d->x, d->status,
                       d->iters, d->x0, d->ref, d->foot, d->last_state, d->alpha_buf, d->plan_table, d->traj,
                       d->status_log, d->iters_log, d->x_log);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

// t.obs_radius (srb_sizes; null: the centre distances and the 0.5 m fail test, the kernels as ever); t.agent_body and
// t.collide_cycle (srb_agent_sizes; body null: d_agent by centres, the kernels as ever; else the kernels of
// srb_agents.hip, which take the radius null or not)
static int launch_metrics(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, hipStream_t s, const SrbTables &t)
{
    const double *radius = t.obs_radius, *body = t.agent_body;
    int *collide = t.collide_cycle;
    if (!d->state) return fail(SRB_ERR_ARG, "srb_sim: missing buffer (state)");
    if (d->n_obs < 0 || d->n_all < 0 || (d->n_obs > 0 && !d->obstacles) || (d->n_all > 0 && !d->nbr_state))
        return fail(SRB_ERR_ARG, "srb_sim: obstacles / nbr_state missing for n_obs / n_all rows");
    // scenes: blocks of one scene each, from the scene of the batch's first agent to that of its last
    if (body && (d->agent_offset < 0 || d->agent_offset + n_agents > d->n_all))
        return fail(SRB_ERR_ARG, "srb_agent_sizes.agent_body: agent_offset + n_agents exceeds n_all (the table's rows)");
    int n_scenes = 0;
    if (int rc = check_scenes(c, n_agents, d->n_obs, d->n_all > 0, d->n_all, d->agent_offset, &n_scenes)) return rc;
    if (n_scenes > 0) {
        const int sa = c->scene_agents, bps = (sa + SRB_SIM_AGENTS_PER_BLOCK - 1) / SRB_SIM_AGENTS_PER_BLOCK;
        const int s0 = d->agent_offset / sa, s1 = (d->agent_offset + n_agents - 1) / sa;
        if (body)
            hipLaunchKernelGGL(srb_sim_scene_metrics_agents_kernel, dim3((s1 - s0 + 1) * bps), dim3(256), 0, s, n_agents,
                               cycle, d->c_first, (const double *)d->state, d->obstacles, radius,
                               d->n_obs > 0 ? c->scene_obs : 0, d->nbr_state, body, d->n_all > 0 ? sa : 0, sa,
                               d->agent_offset, s0, bps, d->d_obs, d->d_agent, d->min_d_obs, d->min_d_agent, d->fail_cycle,
                               d->distance_to_fail, collide);
        else if (radius)
            hipLaunchKernelGGL(srb_sim_scene_metrics_sized_kernel, dim3((s1 - s0 + 1) * bps), dim3(256), 0, s, n_agents,
                               cycle, d->c_first, (const double *)d->state, d->obstacles, radius,
                               d->n_obs > 0 ? c->scene_obs : 0, d->nbr_state, d->n_all > 0 ? sa : 0, sa, d->agent_offset, s0,
                               bps, d->d_obs, d->d_agent, d->min_d_obs, d->min_d_agent, d->fail_cycle, d->distance_to_fail);
        else
            hipLaunchKernelGGL(srb_sim_scene_metrics_kernel, dim3((s1 - s0 + 1) * bps), dim3(256), 0, s, n_agents, cycle,
                               d->c_first, (const double *)d->state, d->obstacles, d->n_obs > 0 ? c->scene_obs : 0,
                               d->nbr_state, d->n_all > 0 ? sa : 0, sa, d->agent_offset, s0, bps, d->d_obs, d->d_agent,
                               d->min_d_obs, d->min_d_agent, d->fail_cycle, d->distance_to_fail);
        HIPCHK(hipGetLastError());
        return SRB_OK;
    }
    if (body)
        hipLaunchKernelGGL(srb_sim_metrics_agents_kernel,
                           dim3((n_agents + SRB_SIM_AGENTS_PER_BLOCK - 1) / SRB_SIM_AGENTS_PER_BLOCK), dim3(256), 0, s,
                           n_agents, cycle, d->c_first, (const double *)d->state, d->obstacles, radius, d->n_obs,
                           d->nbr_state, body, d->n_all, d->agent_offset, d->d_obs, d->d_agent, d->min_d_obs,
                           d->min_d_agent, d->fail_cycle, d->distance_to_fail, collide);
    else if (radius)
        hipLaunchKernelGGL(srb_sim_metrics_sized_kernel,
                           dim3((n_agents + SRB_SIM_AGENTS_PER_BLOCK - 1) / SRB_SIM_AGENTS_PER_BLOCK), dim3(256), 0, s,
                           n_agents, cycle, d->c_first, (const double *)d->state, d->obstacles, radius, d->n_obs,
                           d->nbr_state, d->n_all, d->agent_offset, d->d_obs, d->d_agent, d->min_d_obs, d->min_d_agent,
                           d->fail_cycle, d->distance_to_fail);
    else
        hipLaunchKernelGGL(srb_sim_metrics_kernel,
                           dim3((n_agents + SRB_SIM_AGENTS_PER_BLOCK - 1) / SRB_SIM_AGENTS_PER_BLOCK), dim3(256), 0, s,
                           n_agents, cycle, d->c_first, (const double *)d->state, d->obstacles, d->n_obs, d->nbr_state,
                           d->n_all, d->agent_offset, d->d_obs, d->d_agent, d->min_d_obs, d->min_d_agent, d->fail_cycle,
                           d->distance_to_fail);
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

int srb_internal_sim_metrics(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, hipStream_t s, const SrbTables &t)
{
    return launch_metrics(c, n_agents, d, cycle, s, t);
}

template <bool advance>
static int sim_call(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, void *stream, const srb_sizes *sz,
                    const srb_agent_sizes *ag, const srb_plant *pl)
{
    if (int rc = check_sim(d, cycle, advance)) return rc;
    if (int rc = check_plant(pl, d->x != nullptr)) return rc;
    if (!plant_on(pl)) pl = nullptr;
    if (int rc = srb_check_sizes(sz)) return rc;
    if (int rc = srb_check_agent_sizes(ag, d->nbr_state && d->n_all > 0)) return rc;
    if (!c) return fail(SRB_ERR_ARG, "null argument");
    if (n_agents < 0 || n_agents > c->max_agents) return fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] {
        return advance ? launch_advance(c, n_agents, d, cycle, s, pl)
                       : launch_metrics(c, n_agents, d, cycle, s, srb_tables(nullptr, sz, ag));
    });
}

extern "C" int srb_sim_advance_plant_device(srb_ctx *c, int n_agents, const srb_sim *d, const srb_plant *pl, int cycle,
                                            void *stream)
{
    return sim_call<true>(c, n_agents, d, cycle, stream, nullptr, nullptr, pl);
}

extern "C" int srb_sim_advance_device(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, void *stream)
{
    return srb_sim_advance_plant_device(c, n_agents, d, nullptr, cycle, stream);
}

extern "C" int srb_sim_metrics_agents_device(srb_ctx *c, int n_agents, const srb_sim *d, const srb_sizes *sz,
                                             const srb_agent_sizes *ag, int cycle, void *stream)
{
    return sim_call<false>(c, n_agents, d, cycle, stream, sz, ag, nullptr);
}

extern "C" int srb_sim_metrics_sized_device(srb_ctx *c, int n_agents, const srb_sim *d, const srb_sizes *sz, int cycle,
                                            void *stream)
{
    return srb_sim_metrics_agents_device(c, n_agents, d, sz, nullptr, cycle, stream);
}

extern "C" int srb_sim_metrics_device(srb_ctx *c, int n_agents, const srb_sim *d, int cycle, void *stream)
{
    return srb_sim_metrics_sized_device(c, n_agents, d, nullptr, cycle, stream);
}

// ---- degraded neighbour link (srb_link.hip).  What needs no context -- "the struct degrades the link at all" and the
// argument errors before anything is launched -- is srb_host.h's, shared with the SRB-12 mode
static bool link_on(const srb_link *ln) { return srb_link_on(ln); }
static int check_link(const srb_link *ln, int n_all, const double *last_state, const double *plan_table)
{
    return srb_check_link(ln, n_all, last_state, plan_table);
}

// ... and those that need the context: the plan ranges (N) and the selection that reads the agent's own table row.
// plan: the solve's plan output (srb_batch.plan) or null
static int check_link_ctx(const srb_ctx *c, const srb_link *ln, int n_all, const double *plan_table, const double *plan)
{
    if (!link_on(ln)) return SRB_OK;
    if (c->plan_selection)
        return fail(SRB_ERR_ARG, "SRB_OPT_PLAN_SELECTION = 1 with a srb_link that is on: the horizon-aware selection reads "
                                 "the agent's own previous plan from its row of the table, which would be a stale copy "
                                 "(not built)");
    if (plan_table && c->p.N < 2) return fail(SRB_ERR_ARG, "srb_link: a plan table needs N >= 2 (the plan shift)");
    const size_t rows = (size_t)std::max(n_all, 0) * 2 * c->p.N;
    if (srb_overlap(ln->seen_plan, rows, plan_table, rows))
        return fail(SRB_ERR_ARG, "srb_link.seen_plan overlaps plan_table (the truth the next cycle's messages carry: use "
                                 "two buffers)");
    if (srb_overlap(ln->seen_plan, rows, plan, rows))
        return fail(SRB_ERR_ARG, "srb_link.seen_plan overlaps srb_batch.plan (the solve reads the table while it writes "
                                 "its plans: use two buffers)");
    return SRB_OK;
}

// one cycle's update (launch only: the caller orders the stream); ln is on
static int launch_link(srb_ctx *c, int n_all, const srb_link *ln, const double *last_state, const double *plan_table,
                       int cycle, int c_first, hipStream_t s, int lanes = SRB_LINK_LANES)
{
    const int slot = (int)(((long long)cycle - c_first) % (ln->max_delay + 1));
    int *age_row = ln->age_log ? ln->age_log + (size_t)(cycle - c_first) * (size_t)n_all : nullptr;
    if (srb_launch_link_update(lanes, n_all, c->p.N, c->p.Ts, cycle, c_first, ln->max_delay, slot, ln->extrapolate,
                               (unsigned)(ln->seed & 0xffffffffull), (unsigned)(ln->seed >> 32), ln->delay, ln->drop,
                               ln->noise_p, ln->noise_v, last_state, plan_table, ln->ring_state, ln->ring_plan,
                               ln->held_state, ln->held_plan, ln->held_cycle, ln->seen_state, ln->seen_plan, age_row, s))
        return fail(SRB_ERR_ARG, "srb_link_update_lanes_device: lanes is 1, 8 or 16");
    HIPCHK(hipGetLastError());
    return SRB_OK;
}

extern "C" int srb_link_update_lanes_device(srb_ctx *c, int n_all, const srb_link *ln, const double *last_state,
                                            const double *plan_table, int cycle, int c_first, int lanes, void *stream)
{
    if (int rc = check_link(ln, n_all, last_state, plan_table)) return rc;
    if (cycle < c_first) return fail(SRB_ERR_ARG, "srb_link: cycle precedes c_first");
    if (lanes != 1 && lanes != 8 && lanes != 16) return fail(SRB_ERR_ARG, "srb_link_update_lanes_device: lanes is 1, 8 or 16");
    if (!c) return fail(SRB_ERR_ARG, "null argument");
    if (n_all < 0) return fail(SRB_ERR_ARG, "srb_link: negative n_all");
    if (int rc = check_link_ctx(c, ln, n_all, plan_table, nullptr)) return rc;
    if (!link_on(ln) || n_all == 0) return SRB_OK;
    if (!last_state) return fail(SRB_ERR_ARG, "srb_link: last_state missing");
    hipStream_t s = (hipStream_t)stream;
    return c->order.run(c->device, s, [&] { return launch_link(c, n_all, ln, last_state, plan_table, cycle, c_first, s, lanes); });
}

extern "C" int srb_link_update_device(srb_ctx *c, int n_all, const srb_link *ln, const double *last_state,
                                      const double *plan_table, int cycle, int c_first, void *stream)
{
    return srb_link_update_lanes_device(c, n_all, ln, last_state, plan_table, cycle, c_first, SRB_LINK_LANES, stream);
}

// The driver.  The tables of srb_sizes, srb_agent_sizes, srb_plant and srb_link do not change over a rollout: the same
// pointers serve every cycle.  (The entry points below are this one without a struct: one path.)
extern "C" int srb_rollout_link_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d,
                                       const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                                       const srb_plant *pl, const srb_link *ln, int cycles, void *stream)
{
    if (int rc0 = srb_check_struct(b, "srb_batch")) return rc0;
    if (int rc0 = check_tables(mv, sz, ag, b, true)) return rc0;
    if (int rc0 = check_plant(pl, true)) return rc0;              // (batch.x missing is reported below, as ever)
    if (!plant_on(pl)) pl = nullptr;
    // (the layout and null checks of check_sim only: the driver's first cycle is c_first itself)
    if (int rc = check_sim(d, d && d->struct_size == (int)sizeof(srb_sim) ? d->c_first : 0, false)) return rc;
    if (int rc0 = check_link(ln, n_agents, d->last_state, d->plan_table)) return rc0;
    if (!b) return fail(SRB_ERR_ARG, "null argument");
    if (!d->goal) return fail(SRB_ERR_ARG, "srb_sim.goal missing");
    if (!c) return fail(SRB_ERR_ARG, "null argument");
    if (cycles < 0) return fail(SRB_ERR_ARG, "negative cycles");
    if (n_agents < 0 || n_agents > c->max_agents) return fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (b->agent_offset != 0 || d->agent_offset != 0 || (b->n_all != 0 && b->n_all != n_agents) ||
        (d->n_all != 0 && d->n_all != n_agents))
        return fail(SRB_ERR_ARG, "srb_rollout_device rolls out a whole team on one GPU: a sharded batch (agent_offset != 0 "
                                 "or n_all != n_agents) needs the neighbour exchange between advance and metrics");
    if (srb_overlap(b->plan, (size_t)n_agents * 2 * c->p.N, d->plan_table, (size_t)n_agents * 2 * c->p.N))
        return fail(SRB_ERR_ARG, "srb_sim.plan_table overlaps srb_batch.plan (the solve reads the table while it writes "
                                 "its plans: use two buffers)");
    if (int rc0 = check_link_ctx(c, ln, n_agents, d->plan_table, b->plan)) return rc0;
    if (!link_on(ln)) ln = nullptr;
    if (c->scene_agents > 0) {
        if (n_agents % c->scene_agents != 0)
            return fail(SRB_ERR_ARG, "scenes: srb_rollout_device rolls out whole scenes, n_agents (" + std::to_string(n_agents) +
                                     ") is not a multiple of scene_agents (" + std::to_string(c->scene_agents) + ")");
        if (int rc = check_scenes(c, n_agents, b->n_obs, true, n_agents, 0)) return rc;
    }
    if (n_agents == 0) return SRB_OK;
    // the two structs wired together (include/srbnmpc.h): the solve reads what the advance wrote and back
    srb_sim sim = *d;
    sim.x = b->x; sim.status = b->status; sim.iters = b->iters;
    sim.obstacles = b->obstacles; sim.n_obs = b->n_obs;
    sim.nbr_state = d->last_state; sim.n_all = n_agents; sim.agent_offset = 0;
    srb_batch bat = *b;
    bat.x0 = d->x0; bat.ref = d->ref; bat.foot = d->foot;
    bat.nbr_state = d->last_state; bat.n_all = n_agents; bat.agent_offset = 0;
    bat.alpha_buf = b->alpha ? d->alpha_buf : nullptr;
    if (ln) bat.nbr_state = ln->seen_state;               // the solve reads what is seen, the metrics the truth
    if (!sim.x) return fail(SRB_ERR_ARG, "srb_batch.x missing");
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
        rc = launch_advance(c, n_agents, &sim, cyc, s, pl);
        if (rc || i == cycles) break;
        if (i > 0 && t.obs_vel) rc = srb_launch_obstacles_advance(b->n_obs, c->p.Ts, mv->obstacles, t.obs_vel, s);
        if (!rc) rc = launch_metrics(c, n_agents, &sim, cyc, s, t);
        if (!rc && ln) rc = launch_link(c, n_agents, ln, d->last_state, d->plan_table, cyc, d->c_first, s);
        if (i > 0 && d->plan_table) bat.nbr_plan = ln ? ln->seen_plan : d->plan_table;
        if (!rc) rc = launch(c, n_agents, &bat, s, c->p.use_nlp, t);
    }
    const int rc_mark = c->order.mark_done(s);            // also after a refusal inside the loop: earlier launches run
    return rc ? rc : rc_mark;
}

extern "C" int srb_rollout_plant_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d,
                                        const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag,
                                        const srb_plant *pl, int cycles, void *stream)
{
    return srb_rollout_link_device(c, n_agents, b, d, mv, sz, ag, pl, nullptr, cycles, stream);
}

extern "C" int srb_rollout_agents_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d,
                                         const srb_moving *mv, const srb_sizes *sz, const srb_agent_sizes *ag, int cycles,
                                         void *stream)
{
    return srb_rollout_plant_device(c, n_agents, b, d, mv, sz, ag, nullptr, cycles, stream);
}

extern "C" int srb_rollout_sized_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d,
                                        const srb_moving *mv, const srb_sizes *sz, int cycles, void *stream)
{
    return srb_rollout_agents_device(c, n_agents, b, d, mv, sz, nullptr, cycles, stream);
}

extern "C" int srb_rollout_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d, int cycles, void *stream)
{
    return srb_rollout_sized_device(c, n_agents, b, d, nullptr, nullptr, cycles, stream);
}

extern "C" int srb_rollout_moving_device(srb_ctx *c, int n_agents, const srb_batch *b, const srb_sim *d,
                                         const srb_moving *mv, int cycles, void *stream)
{
    return srb_rollout_sized_device(c, n_agents, b, d, mv, nullptr, cycles, stream);
}

// swarms up to this many agents run as one persistent workgroup (srb_hlplan_kernel); larger ones
// one launch per step over NA / 64 workgroups (srb_hlplan_step_kernel)
#define SRB_HL_ONE_WG 1024

extern "C" int srb_hl_plan(int device, int NA, const double *Pstart, const double *Pobs, int n_obs, int loop, double *Pr,
                           double *Prd)
{
    if (NA < 1 || NA > (1 << 20)) return fail(SRB_ERR_SIZE, "HL planner: 1 <= NA <= 2^20");
    if (n_obs < 0 || n_obs > 2048 || (n_obs > 0 && !Pobs)) return fail(SRB_ERR_ARG, "HL planner: bad obstacle table");
    if (loop < 80 || !Pstart || !Pr || !Prd) return fail(SRB_ERR_ARG, "HL planner: bad arguments (loop >= 80)");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SRB_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    const int T = loop / 40;
    const size_t out = (size_t)T * 2 * NA * sizeof(double);
    double *dPs = nullptr, *dOb = nullptr, *dPr = nullptr, *dPrd = nullptr;
    int rc = SRB_OK;
    auto chk = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == SRB_OK) rc = fail(SRB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    chk(hipMalloc(&dPs, 2 * NA * sizeof(double)), "hipMalloc");
    chk(hipMalloc(&dOb, (n_obs > 0 ? n_obs : 1) * 2 * sizeof(double)), "hipMalloc");
    chk(hipMalloc(&dPr, out), "hipMalloc");
    chk(hipMalloc(&dPrd, out), "hipMalloc");
    if (rc == SRB_OK) {
        chk(hipMemcpy(dPs, Pstart, 2 * NA * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        if (n_obs > 0) chk(hipMemcpy(dOb, Pobs, n_obs * 2 * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
    }
    if (rc == SRB_OK && NA <= SRB_HL_ONE_WG) {
        const int threads = ((NA + 63) / 64) * 64;
        const size_t lds = (4 * (size_t)NA + 2 * (size_t)n_obs) * sizeof(double);
        hipLaunchKernelGGL(srb_hlplan_kernel, dim3(1), dim3(threads), lds, 0, NA, dPs, dOb, n_obs, loop, dPr, dPrd);
        chk(hipGetLastError(), "srb_hlplan_kernel");
        chk(hipDeviceSynchronize(), "srb_hlplan_kernel");
    } else if (rc == SRB_OK) {
        // one coupled swarm across the chip: positions double-buffered in global memory
        double *pos[2] = {nullptr, nullptr}, *st = nullptr;
        chk(hipMalloc(&pos[0], 2 * (size_t)NA * sizeof(double)), "hipMalloc");
        chk(hipMalloc(&pos[1], 2 * (size_t)NA * sizeof(double)), "hipMalloc");
        chk(hipMalloc(&st, 4 * (size_t)NA * sizeof(double)), "hipMalloc");
        if (rc == SRB_OK) {
            double *h = (double *)std::calloc(4 * (size_t)NA, sizeof(double));
            for (int a = 0; a < NA; a++) { h[4 * a] = Pstart[2 * a]; h[4 * a + 1] = Pstart[2 * a + 1]; }
            chk(hipMemcpy(st, h, 4 * (size_t)NA * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
            chk(hipMemcpy(pos[0], Pstart, 2 * (size_t)NA * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
            std::free(h);
        }
        const int blocks = (NA + 63) / 64;
        for (int i = 0; i <= loop && rc == SRB_OK; i++) {
            hipLaunchKernelGGL(srb_hlplan_step_kernel, dim3(blocks), dim3(64), 0, 0, NA, i, loop, dOb, n_obs, pos[i & 1],
                               pos[(i & 1) ^ 1], st, dPr, dPrd);
            if ((i & 1023) == 0) chk(hipGetLastError(), "srb_hlplan_step_kernel");
        }
        chk(hipDeviceSynchronize(), "srb_hlplan_step_kernel");
        for (void *b : {(void *)pos[0], (void *)pos[1], (void *)st})
            if (b) (void)hipFree(b);
    }
    if (rc == SRB_OK) {
        chk(hipMemcpy(Pr, dPr, out, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(Prd, dPrd, out, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    for (void *b : {(void *)dPs, (void *)dOb, (void *)dPr, (void *)dPrd})
        if (b) (void)hipFree(b);
    return rc;
}

extern "C" int srb_sync(srb_ctx *c)
{
    if (!c) return fail(SRB_ERR_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    return SRB_OK;
}

extern "C" int srb_last_kernel_ms(srb_ctx *c, float *knn_ms, float *solve_ms)
{
    if (!c || !c->timed) return fail(SRB_ERR_ARG, "no timed launch");
    HIPCHK(hipEventSynchronize(c->ev[1]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev[0], c->ev[2]));
    HIPCHK(hipEventElapsedTime(&b, c->ev[2], c->ev[3]));
    if (knn_ms) *knn_ms = a;            // srb_knn_kernel (0 when there is nothing to select)
    if (solve_ms) *solve_ms = b;        // srb_nmpc_kernel_*
    return SRB_OK;
}

extern "C" int srb_last_polish_ms(srb_ctx *c, float *polish_ms)
{
    if (!c || !c->timed) return fail(SRB_ERR_ARG, "no timed launch");
    HIPCHK(hipEventSynchronize(c->ev[1]));
    float t = 0;
    if (c->last_polish == 1) HIPCHK(hipEventElapsedTime(&t, c->ev[3], c->ev[1]));
    if (polish_ms) *polish_ms = t;      // srb_polish_kernel_* (0 without it: no NLP stage, or fused)
    return SRB_OK;
}

static int solve_host(srb_ctx *c, int n_agents, const srb_batch *h, int use_nlp, const srb_moving *mv = nullptr,
                      const srb_sizes *sz = nullptr, const srb_agent_sizes *ag = nullptr)
{
    if (int rc0 = srb_check_struct(h, "srb_batch")) return rc0;   // first: it needs no context
    if (int rc0 = check_tables(mv, sz, ag, h, false)) return rc0;
    if (!c || !h) return fail(SRB_ERR_ARG, "null argument");
    if (n_agents < 0 || n_agents > c->max_agents) return fail(SRB_ERR_ARG, "n_agents exceeds max_agents");
    if (n_agents == 0) return SRB_OK;
    const srb_params *p = &c->p;
    const int N = p->N, C = p->C, nv = srb_nv(p);
    const size_t A = (size_t)n_agents;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (int rc0 = c->order.order_after_last(s)) return rc0;   // after the last device launch on this context
    if (int rc0 = check_scenes(c, n_agents, h->obstacles ? h->n_obs : 0, h->n_all > 0 && h->nbr_state, h->n_all, h->agent_offset))
        return rc0;                                           // before the staging copies
    if (!h->x0 || !h->ref || !h->foot || !h->x || !h->obj || !h->status || !h->iters)
        return fail(SRB_ERR_ARG, "missing buffer");
    HIPCHK(hipMemcpyAsync(c->x0, h->x0, A * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->ref, h->ref, A * 4 * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->foot, h->foot, A * 2 * C * N * sizeof(double), hipMemcpyHostToDevice, s));
    srb_batch d = *h;
    d.x0 = c->x0; d.ref = c->ref; d.foot = c->foot;
    d.x_qp = c->x_qp; d.x = c->x; d.obj = c->obj; d.status = c->status; d.iters = c->iters;
    d.alpha_buf = nullptr; d.alpha = nullptr;
    if (h->alpha && h->alpha_buf) {
        HIPCHK(hipMemcpyAsync(c->abuf, h->alpha_buf, A * 4 * sizeof(double), hipMemcpyHostToDevice, s));
        d.alpha_buf = c->abuf; d.alpha = c->alpha;
    } else if (h->alpha || h->alpha_buf) {
        return fail(SRB_ERR_ARG, "alpha and alpha_buf go together (both or neither)");
    }
    d.obstacles = nullptr; d.nbr_state = nullptr;
    if (h->n_obs > 0 && h->obstacles) {
        if (int rc0 = srb_stage_copy(c->order, c->obstacles, c->cap_obs, h->obstacles, (size_t)h->n_obs * 2 * sizeof(double), s))
            return rc0;
        d.obstacles = c->obstacles;
    }
    if (h->n_all > 0 && h->nbr_state) {
        if (int rc0 = srb_stage_copy(c->order, c->nbr, c->cap_nbr, h->nbr_state, (size_t)h->n_all * 4 * sizeof(double), s))
            return rc0;
        d.nbr_state = c->nbr;
    }
    // the plan members: the table staged like nbr_state (NLP stage only), the plans like x
    d.nbr_plan = nullptr;
    if (use_nlp)                           // the overlap rule holds for the caller's own (host) buffers
        if (int rc0 = check_plans(c, n_agents, h, false)) return rc0;
    if (use_nlp && h->nbr_plan && d.nbr_state) {
        if (int rc0 = srb_stage_copy(c->order, c->nbr_plan, c->cap_plan, h->nbr_plan, (size_t)h->n_all * 2 * N * sizeof(double), s))
            return rc0;
        d.nbr_plan = c->nbr_plan;
    }
    d.plan = h->plan ? c->plan : nullptr;
    // The tables: ht the caller's (host), t their staged copies.  The velocity and the level table are staged like
    // the obstacle table they belong to, the agent tables with n_all rows each.  All four only with the NLP stage:
    // srb_solve_qp comes this way and reads none.  (solve_host12 leaves that test out for the first two; there the
    // QP-only solve selects no rows, launch12 then hands neither to a kernel, and nothing observable depends on it.)
    const SrbTables ht = srb_tables(mv, sz, ag);
    SrbTables t = {};
    t.obs_horizon = ht.obs_horizon; t.obs_clear = ht.obs_clear; t.nbr_clear = ht.nbr_clear;
    if (use_nlp && ht.obs_vel && d.obstacles) {
        if (int rc0 = srb_stage_copy(c->order, c->obs_vel, c->cap_vel, ht.obs_vel, (size_t)h->n_obs * 2 * sizeof(double), s))
            return rc0;
        t.obs_vel = c->obs_vel;
    }
    if (use_nlp && ht.obs_eps && d.obstacles) {
        if (int rc0 = srb_stage_copy(c->order, c->obs_eps, c->cap_eps, ht.obs_eps, (size_t)h->n_obs * sizeof(double), s))
            return rc0;
        t.obs_eps = c->obs_eps;
    }
    if (use_nlp && (ht.agent_rad || ht.agent_pad)) {
        if (h->agent_offset < 0 || h->agent_offset + n_agents > h->n_all)    // launch()'s refusal, before the copies
            return fail(SRB_ERR_ARG, "srb_agent_sizes: agent_offset + n_agents exceeds n_all (the agent tables' rows)");
        const size_t bytes = (size_t)h->n_all * sizeof(double);
        if (ht.agent_rad) {
            if (int rc0 = srb_stage_copy(c->order, c->agent_rad, c->cap_rad, ht.agent_rad, bytes, s)) return rc0;
            t.agent_rad = c->agent_rad;
        }
        if (ht.agent_pad) {
            if (int rc0 = srb_stage_copy(c->order, c->agent_pad, c->cap_pad, ht.agent_pad, bytes, s)) return rc0;
            t.agent_pad = c->agent_pad;
        }
    }
    t.normalise();                         // (a table that was not staged takes its flag with it)
    d.sel = nullptr;                       // the context's scratch; copied out below when asked for
    d.obstacles_version = 0;               // staged copy: rebuilt every call
    int rc = launch(c, n_agents, &d, s, use_nlp, t);
    if (!rc) rc = c->order.mark_done(s);
    if (rc) return rc;
    if (h->sel && use_nlp) {
        int Ko = p->K_obs, Kn = p->K_nbr;
        clamp_K(c, h->n_obs, h->nbr_state && h->n_all > 0, h->n_all, &Ko, &Kn);       // as launch() did on the staged tables
        if (Ko + Kn > 0) HIPCHK(hipMemcpyAsync(h->sel, c->sel, A * (Ko + Kn) * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (h->x_qp) HIPCHK(hipMemcpyAsync(h->x_qp, c->x_qp, A * nv * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->x, c->x, A * nv * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->obj, c->obj, A * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->status, c->status, A * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->iters, c->iters, A * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (d.alpha) HIPCHK(hipMemcpyAsync(h->alpha, c->alpha, A * 20 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (d.plan) HIPCHK(hipMemcpyAsync(h->plan, c->plan, A * 2 * N * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SRB_OK;
}

extern "C" int srb_solve_batch_agents(srb_ctx *c, int n_agents, const srb_batch *host_io, const srb_moving *host_mv,
                                      const srb_sizes *host_sz, const srb_agent_sizes *host_ag)
{
    return solve_host(c, n_agents, host_io, c ? c->p.use_nlp : 0, host_mv, host_sz, host_ag);
}

extern "C" int srb_solve_batch_sized(srb_ctx *c, int n_agents, const srb_batch *host_io, const srb_moving *host_mv,
                                     const srb_sizes *host_sz)
{
    return srb_solve_batch_agents(c, n_agents, host_io, host_mv, host_sz, nullptr);
}

extern "C" int srb_solve_batch(srb_ctx *c, int n_agents, const srb_batch *host_io)
{
    return srb_solve_batch_sized(c, n_agents, host_io, nullptr, nullptr);
}

extern "C" int srb_solve_qp(srb_ctx *c, int n_agents, const srb_batch *host_io)
{
    return solve_host(c, n_agents, host_io, 0);
}

extern "C" int srb_solve_batch_moving(srb_ctx *c, int n_agents, const srb_batch *host_io, const srb_moving *host_mv)
{
    return srb_solve_batch_sized(c, n_agents, host_io, host_mv, nullptr);
}

// fitComTrajectory_eventbase (MPC_dist.cpp:784-855).  With N == NDOMAIN the reference's
// 24x24 KKT (whose 20x8 -> 20x4 block assignment keeps only the s = 0 end-point row)
// has the unique solution of the 5-point Bernstein interpolation through
// [buf, X0, X1, X2, X3] at s = 0, 1/4, 1/2, 3/4, 1, solved here per state row.
extern "C" void srb_fit_bezier(const double buf[4], const double *X, double alpha[20])
{
    static const double binom[5] = {1, 4, 6, 4, 1};
    for (int d = 0; d < 4; d++) {
        double M[5][6];
        for (int i = 0; i < 5; i++) {
            double s = i * 0.25;
            for (int j = 0; j < 5; j++) M[i][j] = binom[j] * std::pow(s, j) * std::pow(1 - s, 4 - j);
            M[i][5] = (i == 0) ? buf[d] : X[(i - 1) * 4 + d];
        }
        for (int k = 0; k < 5; k++) {           // Gaussian elimination, partial pivoting
            int piv = k;
            for (int i = k + 1; i < 5; i++) if (std::fabs(M[i][k]) > std::fabs(M[piv][k])) piv = i;
            if (piv != k) for (int j = 0; j < 6; j++) std::swap(M[k][j], M[piv][j]);
            for (int i = k + 1; i < 5; i++) {
                double l = M[i][k] / M[k][k];
                for (int j = k; j < 6; j++) M[i][j] -= l * M[k][j];
            }
        }
        double a[5];
        for (int i = 4; i >= 0; i--) {
            double s = M[i][5];
            for (int j = i + 1; j < 5; j++) s -= M[i][j] * a[j];
            a[i] = s / M[i][i];
        }
        for (int j = 0; j < 5; j++) alpha[d * 5 + j] = a[j];
    }
}

extern "C" const char *srb_last_error(void) { return g_err.c_str(); }

#ifdef SRB_NLPDBG
extern __device__ double srb_nlp_dbg[SRB_NLP_DBG_LEN];
extern __device__ int srb_nlp_dbg_agent;
// diagnostic build only: select the traced agent (-1: none) and read/clear the trace
extern "C" int srb_debug_nlp_trace(int agent, double *out)
{
    HIPCHK(hipDeviceSynchronize());
    if (out) HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(srb_nlp_dbg), sizeof(double) * SRB_NLP_DBG_LEN));
    double z[SRB_NLP_DBG_LEN] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(srb_nlp_dbg), z, sizeof z));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(srb_nlp_dbg_agent), &agent, sizeof(int)));
    return SRB_OK;
}
#endif

#ifdef SRB_STAMPS
extern __device__ unsigned long long srb_stamp_buf[64];
extern "C" int srb_debug_stamps(unsigned long long *out, int reset)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(srb_stamp_buf), sizeof(unsigned long long) * 64));
    if (reset) {
        unsigned long long z[64] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(srb_stamp_buf), z, sizeof z));
    }
    return SRB_OK;
}
#endif
