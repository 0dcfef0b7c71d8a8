// Batched CBF-NMPC solver kernel for MI355X (gfx950).
//
// Replaces the per-control-cycle solve of MPC_dist::run_NMPC
// (/root/reference/src/MPC_dist.cpp:81-454): the LIP/CoP/contact-weight QP of :135-321
// solved with the iSWIFT Mehrotra predictor-corrector
// (/root/reference/optimization/iSWIFT/src/Prime.c:127-230), then the NLP stage with the
// obstacle ("CBF") and velocity rows of include/dec_vars_constr_cost.h:245-395 (SNOPT in
// the reference) solved by a primal-dual interior-point method warm-started from the QP
// solution (MPC_dist.cpp:403).
//
// Execution model: one 64-lane wavefront (= one workgroup) per agent runs the whole path
// -- nearest-obstacle selection, problem setup, both interior-point loops, output -- with
// no host round trip.  The solve is latency-bound (a few thousand dependent instructions
// per IPM iteration on one wave), so the design minimises instructions and LDS round
// trips per iteration:
//
//   * equalities (LIP dynamics, u_k = F_k lambda_k, sum lambda_k = 1) are eliminated by a
//     null-space basis: x = xbar + Z xi, xi = (lambda dofs of every grid, s),
//     nz = N(C-1)+1 (11 at N=10 trot);
//   * every inequality row lives in REGISTERS of a fixed owner lane for the whole solve:
//       - variable slot v (lane v % 64, trip v / 64): x_v, the residual rx_v and the two
//         bound pairs on x_v (A: box / lambda in [0,1]; B: velocity, NLP only);
//       - CoM-CoP slot e: the pair +-(p_i - u_{i+1}) <= mu h / sqrt 2 (row M_e = a_e'Z in LDS);
//       - obstacle slot o = k*K + j: -|p_k - o_kj|^2 - s <= -eps (row M_o = J_o Z in LDS,
//         re-linearised every iteration);
//     so residuals, step lengths and updates are straight-line VALU code with no branches
//     on row type;
//   * the reduced Newton matrix  Z'HZ = sum_t w_t r_t r_t'  over the term rows r_t (Z rows
//     of the variables with their diagonal weights, M_e, M_o) is assembled on the matrix
//     cores (v_mfma_f64_16x16x4f64, LDS operands), inverted by Gauss-Jordan with one matrix
//     row per lane and v_readlane broadcasts (no LDS inside the elimination), and every
//     Newton solve is two register matvecs plus one refinement;
//   * right-hand sides Z'(rx + J'w) are VALU dot products over the same term rows followed
//     by a permlane butterfly; J dx of every slot is its LDS term row dotted with dxi;
//   * rx is carried by the exact recurrence of the iSWIFT update (q += ad A'dy):
//       rx' = (1-ad) rx + (ad-ap) P dx + ad (hess + delta) dx - (J(x') - J(x))' z'
//     so neither J'z nor the equality multipliers are ever formed.
//
// Inputs/outputs are agent-major fp64 arrays in HBM, read once / written once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "srb_kernel_params.h"
#include "srb_kernel_decls.h"

#define WAVE 64
#include "srb_wave.h"
#include "srb_gj.h"
#include "srb_solve.h"
#include "srb_gram.h"
#define SYNC() srb_sync<NW>()       // the workgroup barrier of srb_wave.h (every SYNC site sits in a function templated on NW)

// --------------------------------------------------------------------------- diagnostic stamps
// Built only with -DSRB_STAMPS (make stamps -> srbnmpc/libsrbnmpc_stamps.so): lane 0 of
// every agent accumulates s_memtime cycles per phase into registers; agent 0 adds them to
// a device buffer nothing else reads.
#ifdef SRB_STAMPS
#define SRB_NSTAMP 64
__device__ unsigned long long srb_stamp_buf[SRB_NSTAMP];
#define STAMP_DECL unsigned long long st_t0 = 0; int st_off = 0
#define STAMP_BEGIN() do { __builtin_amdgcn_sched_barrier(0); st_t0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_END(slot) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long _t = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0); if (threadIdx.x == 0 && stamp_lds) atomicAdd(&stamp_lds[st_off + (slot)], _t - st_t0); st_t0 = _t; } while (0)
#define STAMP_STAGE(s) (st_off = 32 * (s))
#define STAMP_FLUSH(agent) do { SYNC(); if ((agent) == 0 && threadIdx.x < 64) atomicAdd(&srb_stamp_buf[threadIdx.x], stamp_lds[threadIdx.x]); } while (0)
#else
#define STAMP_DECL do {} while (0)
#define STAMP_BEGIN() do {} while (0)
#define STAMP_END(slot) do {} while (0)
#define STAMP_STAGE(s) do {} while (0)
#define STAMP_FLUSH(agent) do {} while (0)
#endif

// --------------------------------------------------------------------------- LDS bounds (diagnostic)
// Built only with -DSRB_DIAG_LDS_CHECK (make fullvar TAG=ldsck VARFLAGS=-DSRB_DIAG_LDS_CHECK):
// the indices a slot derives its LDS accesses from -- its term row, weight entry, iterate entries, obstacle and
// dual entries, exported active-set entry --, the term-row ranges of the Gram, and the carve's end against the
// size the host allocated (srb_lds_doubles) are checked, each failed check setting one bit of a workgroup
// flag; a flagged agent reports QP status 1000 + flag (never a fault: the kernel goes on).  Round 5's fold
// build read obstacle term rows past the end of R with four waves -- bit 1 here.
#ifdef SRB_DIAG_LDS_CHECK
#ifndef SRB_DIAG_BUILD
#error "SRB_DIAG_LDS_CHECK is a diagnostic-build option"
#endif
__device__ __forceinline__ int *lds_oob_flag()
{
    __shared__ int f;
    return &f;
}
#define LCK(ok, bit) do { if (!(ok)) __hip_atomic_fetch_or(lds_oob_flag(), 1 << (bit), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } while (0)
#define LCK_INIT() do { if (threadIdx.x == 0) *lds_oob_flag() = 0; } while (0)
#define LCK_REPORT(slot) do { SYNC(); if (tid == 0 && *lds_oob_flag()) status_out[(slot)] = 1000 + *lds_oob_flag(); } while (0)
#else
#define LCK(ok, bit) do {} while (0)
#define LCK_INIT() do {} while (0)
#define LCK_REPORT(slot) do {} while (0)
#endif

// --------------------------------------------------------------------------- diagnostic trace
// Built only with -DSRB_NLPDBG (make nlpdbg -> srbnmpc/libsrbnmpc_nlpdbg.so): agent
// srb_nlp_dbg_agent records, per NLP iteration, ||rx||, its threshold, ||rz||, s'z/m, ap, ad,
// delta and sigma (8 doubles) into srb_nlp_dbg; nothing else reads it.
#ifdef SRB_NLPDBG
__device__ double srb_nlp_dbg[SRB_NLP_DBG_LEN];
__device__ int srb_nlp_dbg_agent = -1;
#define NLPDBG(it, k, v) do { if (nl && agent == srb_nlp_dbg_agent && tid == 0 && (it) < 64) srb_nlp_dbg[8 * (it) + (k)] = (v); } while (0)
// polish kernel: pass p of the traced agent into row 56 + p: primal, |c_A|, -min z_A, max |z_A|,
// max inactive violation, last |dx|, accepted, Newton steps
#define POLDBG(p, k, v) do { if (agent == srb_nlp_dbg_agent && tid == 0 && (p) < 8) srb_nlp_dbg[8 * (56 + (p)) + (k)] = (v); } while (0)
// polish kernel, first Newton step of pass 0: the reduced matrix (32 x 32 at 512) and right-hand
// side (at 512 + 1024) of the traced agent, for an eigenvalue check on the host
// and, at the polish kernel's start, the exported zpol row values (2 S at 1568) and x (at 2592)
#define POLDBG_IN(zp, S, xs, n) do { if (agent == srb_nlp_dbg_agent) { \
    for (int e = tid; e < 2 * (S) && e < 1024; e += NTH) srb_nlp_dbg[1568 + e] = (zp)[e]; \
    for (int e = tid; e < (n) && e < 256; e += NTH) srb_nlp_dbg[2592 + e] = (xs)[e]; } } while (0)
// x after each Newton step of pass 0 (3 x 256 at 2848)
#define POLDBG_X(p, it, xs, n) do { SYNC(); if (agent == srb_nlp_dbg_agent && (p) == 0 && (it) < 3) \
    for (int e = tid; e < (n) && e < 256; e += NTH) srb_nlp_dbg[2848 + 256 * (it) + e] = (xs)[e]; } while (0)
#define POLDBG_MAT(H, LDH, v, nz) do { if (agent == srb_nlp_dbg_agent) \
    for (int e = tid; e < (nz) * (nz); e += NTH) { srb_nlp_dbg[512 + 32 * (e / (nz)) + e % (nz)] = (H)[(e / (nz)) * (LDH) + e % (nz)]; \
        if (e < (nz)) srb_nlp_dbg[512 + 1024 + e] = (v)[e]; } } while (0)
#else
#define POLDBG_MAT(H, LDH, v, nz) do {} while (0)
#define POLDBG_IN(zp, S, xs, n) do {} while (0)
#define POLDBG_X(p, it, xs, n) do {} while (0)
#define NLPDBG(it, k, v) do {} while (0)
#define POLDBG(p, k, v) do {} while (0)
#endif


// Re-linearisation of obstacle row o at x: J_o = (jx, jy, -1) on (p_x(k), p_y(k), slack).  Stored-row
// instances (SRB_OBS_STORED(NZL)) materialise its term row in R, M_o = jx Z_x(k) + jy Z_y(k) - e_s
// (i0 = 4k, i1 = 4k + 2: the grid's CoM rows); the others keep (jx, jy) in OJ for the fold (ObsFold)
template <int NZL>
__device__ __forceinline__ void obs_relin(double *R, double *OJ, int rO, int o, int i0, int i1, double jx, double jy)
{
    if constexpr (SRB_OBS_STORED(NZL)) {
        constexpr int LDR = NZL + 1;
        double *dst = R + (rO + o) * LDR;
        const double *zx = R + i0 * LDR, *zy = R + i1 * LDR;
        // both source rows first: dst, zx and zy all point into R with run-time rows, so a load written after a
        // store could not be moved above it (one dependent LDS round trip an element)
        double vx[NZL], vy[NZL];
#pragma unroll
        for (int a = 0; a < NZL; a++) { vx[a] = zx[a]; vy[a] = zy[a]; }
#pragma unroll
        for (int a = 0; a < NZL; a++) dst[a] = fma(jx, vx[a], fma(jy, vy[a], (a == 0) ? -1.0 : 0.0));
    } else {
        OJ[2 * o] = jx; OJ[2 * o + 1] = jy;
    }
}

// --------------------------------------------------------------------------- null space
// Basis of the per-grid contact-weight directions {d : 1'd = 0} (lambda = e_{C-1} + N xi).
// Columns e_i - e_{C-1}, except for C = 4, where one column is replaced by the exact null
// vector n of [F; 1'] (u = F lambda unchanged): its U and X parts are identically zero, so
// the vanishing curvature along it near convergence (both lambda bounds inactive) is held
// exactly in Z'HZ instead of emerging from cancellation between O(1e3) terms.
// Returns 1 when column t is that null column (lam holds it), 0 otherwise.
// (every index into lam / nvec is a compile-time constant after unrolling: a runtime index would put
// these arrays in scratch memory, 48 B per lane written back to HBM by every launch)
__device__ __forceinline__ int lambda_basis(const double *F, int C, int t, double (&lam)[4])
{
    if (C != 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) lam[i] = (i == t) ? 1.0 : (i == C - 1) ? -1.0 : 0.0;
        return 0;
    }
    double nvec[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c0 = (i == 0) ? 1 : 0, c1 = (i <= 1) ? 2 : 1, c2 = (i <= 2) ? 3 : 2;
        const double *r0 = F, *r1 = F + 4;
        double det = r0[c0] * (r1[c1] - r1[c2]) - r0[c1] * (r1[c0] - r1[c2]) + r0[c2] * (r1[c0] - r1[c1]);
        nvec[i] = (i & 1) ? -det : det;
    }
    int istar = 0;
    if (fabs(nvec[1]) > fabs(nvec[istar])) istar = 1;
    if (fabs(nvec[2]) > fabs(istar == 1 ? nvec[1] : nvec[0])) istar = 2;
    const double sc = 1.0 / (istar == 0 ? nvec[0] : istar == 1 ? nvec[1] : nvec[2]);
    if (t == 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) lam[i] = nvec[i] * sc;
        return 1;
    }
    const int ii = (t < istar) ? t : t + 1;
#pragma unroll
    for (int j = 0; j < 4; j++) lam[j] = (j == ii) ? 1.0 : (j == 3) ? -1.0 : 0.0;
    return 0;
}

// --------------------------------------------------------------------------- slots
// Every inequality row of the problem belongs to a SLOT: a bound pair on one scalar
// function f of x (row 0: f <= h0, row 1: -f <= h1; a single row has row 1 off) whose
// Jacobian, reduced by Z, is one term row of R.  Slot s lives in registers of lane s % 64
// (trip s / 64) for the whole solve.  Kinds, in slot order:
//   VAR  s in [0, n):            f = x_v (v = s), box +-1e3 on X/U, [0, 1] on lambda, none on
//                                the slack; also carries rx_v, P_v, c_v; term row v (Z row)
//   COP  [n, n + 2(N-1)):        f = p_i - u_{i+1}, +-mu h / sqrt 2; term row M_e
//   VEL  [.., + 2N) (NLP):       f = xdot_k / ydot_k, +-vsat; adds into term row v
//   OBS  [.., + N K) (NLP):      f = -|p_k - o_kj|^2 - s, single row <= -eps_j; term row M_o
// so residuals, Newton rows, step lengths and updates are one straight-line code path.
// In a compiled-shape instance the kinds of trip t = s / (64 NW) are known when the kernel is compiled
// (SlotTrips below): e.g. 12_4_1_10_2_11 has trip 0 all VAR, trip 1 mixed, trips 2 and 3 OBS / NONE, and on
// the last two the row-1 fields of the slot (s[1], z[1], ...) are never touched, so they hold no registers.
// (the rule slot -> kind: srb_slot_kind, srb_kernel_params.h)
enum { K_NONE = SRB_K_NONE, K_VAR = SRB_K_VAR, K_COP = SRB_K_COP, K_VEL = SRB_K_VEL, K_OBS = SRB_K_OBS };

struct Slot {
    double s[2], z[2], iz[2], is[2], dz[2], ds[2], dsT[2], r3[2];
    double h[2];        // row bounds
    double a0, a1, rx;  // VAR: P_v, c_v ; OBS: o_x, o_y
    double jd;          // J dx of the latest Newton solve (VAR: dx_v)
    double m[2];        // 1.0 / 0.0: row active in the current stage (arithmetic masks keep
                        // per-lane flags in VGPRs instead of long-lived SGPR lane masks)
    int i0, i1, r;      // xs indices of f, term row
    int wr;             // row this slot stores W / CF to (a scratch entry for VEL / unused slots)
    int kind;
};

// kind read through an opaque copy: comparisons on it are recomputed at each use instead
// of being hoisted into lane masks that stay live across the whole iteration.  The slot passes
// reach it through SlotTrips (below), which answers from the compiled shape's trip table where it can
// and reads the kind only on the trips that mix kinds
__device__ __forceinline__ int kind_of(const Slot &q)
{
    int k = q.kind;
    asm volatile("" : "+v"(k));
    return k;
}

// What the slot passes know at compile time about trip t of an instance (NTH threads per agent, shape NC, CC, KC):
// the slots tid + NTH t of a compiled shape can only be of the kinds srb_trip_kinds gives (srb_kernel_params.h),
// so after the passes' `#pragma unroll` over t
//   - a test for a kind that cannot occur on the trip is false, and a trip of one kind never reads q.kind;
//   - on a trip of single-row kinds (OBS / NONE) row 1 is neither computed nor kept (two(t) false, m(q, t, 1) = 0);
//   - where every slot is a VAR below n - 1 the row masks could be the constant 1 (on(t); switched off, see there).
// A trip of mixed kinds keeps the opaque kind_of() path, and so does every trip of a run-time shape (any kind, two
// rows, masks from q.m): those instances compile to what they were without the table.
template <int NTH, int TS, int NC, int CC, int KC>
struct SlotTrips {
    static_assert(srb_trips_cover(NC, CC, KC, NTH, TS), "slot-kind tables do not cover the slots of a trip");
    static constexpr bool compiled = srb_shape_compiled(NC, CC, KC);
    static __device__ __forceinline__ constexpr int kinds(int t) { return srb_trip_kinds(NC, CC, KC, NTH, t); }
    static __device__ __forceinline__ constexpr bool can(int t, int k) { return (kinds(t) >> k) & 1; }
    static __device__ __forceinline__ constexpr bool only(int t, int k) { return kinds(t) == (1 << k); }
    static __device__ __forceinline__ constexpr bool single(int t) { return (kinds(t) & (kinds(t) - 1)) == 0; }
    static __device__ __forceinline__ constexpr bool two(int t) { return srb_trip_rows(NC, CC, KC, NTH, t) == 2; }
    // both rows on in both stages (srb_trip_all_rows_on: the all-VAR trip).  Not used for the masks: with m = 1 folded
    // into the arithmetic of that trip every product is still exact, but the compiler then pairs some multiply and
    // add of the iteration into a different fma, and 190 of configs[2]'s 1024 agents ended 5e-12 off the bits they
    // had (bisected on the GPU, one part of the table at a time).  The masks of that trip stay in q.m.
    static constexpr bool USE_ALL_ROWS_ON = false;
    static __device__ __forceinline__ constexpr bool on(int t) { return USE_ALL_ROWS_ON && srb_trip_all_rows_on(NC, CC, KC, NTH, t); }
    static __device__ __forceinline__ constexpr bool com(int t) { return srb_trip_has_com(NC, CC, KC, NTH, t); }
    static __device__ __forceinline__ constexpr int the_kind(int t)
    {
        return only(t, K_VAR) ? K_VAR : only(t, K_COP) ? K_COP : only(t, K_VEL) ? K_VEL : only(t, K_OBS) ? K_OBS : K_NONE;
    }
    // the slot's kind for several tests (eq): the trip's one kind, or the opaque / plain read of q.kind
    static __device__ __forceinline__ int kind(const Slot &q, int t) { return single(t) ? the_kind(t) : kind_of(q); }
    static __device__ __forceinline__ constexpr bool eq(int t, int kd, int k) { return can(t, k) && kd == k; }
    // one test (opaque / plain)
    static __device__ __forceinline__ bool is(const Slot &q, int t, int k) { return can(t, k) && (only(t, k) || kind_of(q) == k); }
    static __device__ __forceinline__ bool isp(const Slot &q, int t, int k) { return can(t, k) && (only(t, k) || q.kind == k); }
    // row mask
    static __device__ __forceinline__ double m(const Slot &q, int t, int r) { return on(t) ? 1.0 : (r && !two(t)) ? 0.0 : q.m[r]; }
};

// The slot passes' view of SlotTrips (TK: the pass's instance of it, t: the unrolled trip).  For a run-time shape each
// of these is the plain expression the pass used before the table existed, chosen while the source is parsed
// (TK::compiled is a constant there), so those instances compile to the code they had.
#define SK_IS(q, t, k) (TK::compiled ? TK::is(q, t, k) : kind_of(q) == (k))        /* one kind test, opaque read */
#define SK_ISP(q, t, k) (TK::compiled ? TK::isp(q, t, k) : (q).kind == (k))        /* ... plain read */
#define SK_KIND(q, t) (TK::compiled ? TK::kind(q, t) : kind_of(q))                 /* the kind for several SK_EQ tests */
#define SK_EQ(t, kd, k) (TK::compiled ? TK::eq(t, kd, k) : (kd) == (k))
#define SK_M(q, t, r) (TK::compiled ? TK::m(q, t, r) : (q).m[r])                   /* row mask */
#define SK_TWO(t) (!TK::compiled || TK::two(t))                                    /* row 1 exists on the trip */
#define SK_ON(t) (TK::compiled && TK::on(t))                                       /* both rows on in both stages */
#define SK_COM(t) (!TK::compiled || TK::com(t))                                    /* CoM VAR slots can occur */

// (x0, x1: xs[q.i0], xs[q.i1], loaded by the caller -- the residual loop loads every slot's pair before the
// first slot's arithmetic: the term-row stores of a slot's re-linearisation would hold the next slot's loads back)
template <class TK>
__device__ __forceinline__ double slot_fx(const Slot &q, int t, double x0, double x1, double s_var)
{
    const int k = SK_KIND(q, t);
    const double dx = x0 - q.a0, dy = x1 - q.a1;
    return SK_EQ(t, k, K_OBS) ? -(dx * dx + dy * dy) - s_var : SK_EQ(t, k, K_COP) ? x0 - x1 : x0;
}
template <class TK>
__device__ __forceinline__ double slot_f(const Slot &q, int t, const double *xs, double s_var)
{
    return slot_fx<TK>(q, t, xs[q.i0], xs[q.i1], s_var);
}



// sum_j z_kj over the K obstacle rows of grid k (zo, LDS), in index order: unrolled in chunks of
// 16 with predicated loads, so the loads of a chunk are in flight together instead of one
// dependent load per row
__device__ __forceinline__ double zo_sum(const double *zo, int k, int K)
{
    const double *z = zo + k * K;
    double s = 0.0;
    for (int j0 = 0; j0 < K; j0 += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = (j0 + u < K) ? z[j0 + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) s += v[u];
    }
    return s;
}

// Slot sl's constants (kind, function indices, term row, bounds, cost terms); see Slot.
__device__ __forceinline__ void slot_init(Slot &q, int sl, const SrbKParams &prm, const TermLayout &TL, const double *ref,
                                          int sE, int sV, int sO, int S, int rC, int rO, int K, int TT)
{
    const int N = prm.N, n = prm.n;
    q.kind = K_NONE; q.i0 = q.i1 = 0; q.r = 0; q.h[0] = q.h[1] = 0.0; q.a0 = q.a1 = 0.0; q.rx = 0.0; q.jd = 0.0;
    q.m[0] = q.m[1] = 0.0; q.wr = TT;
    if (sl < SRB_SLOT_END(K_VAR, sE, sV, sO, S)) {
        const int v = sl;
        const bool isX = v < 4 * N, isU = !isX && v < 6 * N, isL = !isX && !isU && v < n - 1;
        q.kind = K_VAR; q.i0 = q.i1 = v; q.r = TL.zr(v);
        q.a0 = isX ? ((v >= 4 * (N - 1)) ? prm.Pw : prm.Qw) : isU ? prm.Rw : isL ? 0.0 : prm.Sw;
        q.a1 = isX ? -q.a0 * ref[v] : 0.0;
        q.h[0] = isL ? 1.0 : prm.box; q.h[1] = isL ? 0.0 : prm.box;
    } else if (sl < SRB_SLOT_END(K_COP, sE, sV, sO, S)) {
        const int e = sl - sE, i = e >> 1, d = e & 1;
        q.kind = K_COP; q.i0 = 4 * i + 2 * d; q.i1 = 4 * N + 2 * (i + 1) + d; q.r = rC + e;
        q.h[0] = q.h[1] = prm.fr;
    } else if (sl < SRB_SLOT_END(K_VEL, sE, sV, sO, S)) {
        const int tt = sl - sV, comp = (tt < N) ? 1 : 3, k = tt % N;
        q.kind = K_VEL; q.i0 = q.i1 = 4 * k + comp; q.r = 4 * k + comp;
        q.h[0] = q.h[1] = prm.vsat;
    } else if (sl < SRB_SLOT_END(K_OBS, sE, sV, sO, S)) {                        // (positions filled at the NLP stage)
        const int o = sl - sO, k = o / K;
        q.kind = K_OBS; q.i0 = 4 * k; q.i1 = 4 * k + 2; q.r = rO + o;
    }
#pragma unroll
    for (int r = 0; r < 2; r++) { q.s[r] = q.z[r] = 1.0; q.iz[r] = q.is[r] = 1.0; q.dz[r] = q.ds[r] = q.dsT[r] = q.r3[r] = 0.0; }
}

// the rows of slot q active in the stage (QP: linear rows; NLP: all), and the weight / rhs entry
// it stores to (VEL adds into its variable's term row instead: the scratch entry TT)
template <class TK>
__device__ __forceinline__ void slot_stage(Slot &q, int t, int n, bool nl, int TT)
{
    const bool lin = (SK_ISP(q, t, K_VAR) && (SK_ON(t) || q.i0 < n - 1)) || SK_ISP(q, t, K_COP);
    q.m[0] = (lin || (nl && (SK_ISP(q, t, K_VEL) || SK_ISP(q, t, K_OBS)))) ? 1.0 : 0.0;
    q.m[1] = (lin || (nl && SK_ISP(q, t, K_VEL))) ? 1.0 : 0.0;
    q.wr = (SK_ISP(q, t, K_VAR) || SK_ISP(q, t, K_COP) || SK_ISP(q, t, K_OBS)) ? q.r : TT;
}

// LDS-bounds diagnostic build: the indices slot q (slot number sl) reads and writes through (LCK above)
#define SRB_SLOT_LCK(q, sl) do { \
    LCK((q).wr <= TT, 2); \
    LCK((q).kind == K_NONE || ((q).i0 >= 0 && (q).i0 < n && (q).i1 >= 0 && (q).i1 < n), 3); \
    LCK(!((q).kind == K_VAR || (q).kind == K_COP || (q).kind == K_VEL || ((q).kind == K_OBS && SRB_OBS_STORED(NZL))) || \
        ((q).r >= 0 && (q).r < RROWS), 1); \
    LCK((q).kind != K_OBS || ((sl) - sO >= 0 && (sl) - sO < NK && (q).r - rO == (sl) - sO), 5); \
} while (0)

// cost weight of variable v (Q_qp diagonal, MPC_dist.cpp:168-178)
__device__ __forceinline__ double var_weight(const SrbKParams &prm, int v)
{
    const int N = prm.N;
    return v < 4 * N ? ((v >= 4 * (N - 1)) ? prm.Pw : prm.Qw) : v < 6 * N ? prm.Rw : v < prm.n - 1 ? 0.0 : prm.Sw;
}

// Polish helper: every slot's row function g(x) into q.jd, each obstacle slot's term row M_o
// re-linearised at x (obs_relin: both source rows loaded before the stores) and its multiplier into zo.
template <int NZL, int TS, int NW, class TK>
__device__ __forceinline__ void polish_rows(Slot (&Q)[TS], int nts, const double *xs, double *OJ, double *zo, int n,
                                            int rO, double *R, int nz)
{
    const double s_var = xs[n - 1];
#pragma unroll
    for (int t = 0; t < TS; t++)
        if (t < nts) {
            Slot &q = Q[t];
            q.jd = slot_f<TK>(q, t, xs, s_var);
            if (SK_IS(q, t, K_OBS)) {
                const int o = q.r - rO;
                obs_relin<NZL>(R, OJ, rO, o, q.i0, q.i1, -2.0 * (xs[q.i0] - q.a0), -2.0 * (xs[q.i1] - q.a1));
                zo[o] = q.ds[0] * q.dz[0];
            }
        }
}

// Largest residual, over this thread's grids k = tid, tid + NTH, .., of the equality rows every returned
// point must satisfy (dec_vars_constr_cost.h:154-206): the LIP dynamics X_k = Ad X_{k-1} + Bd U_k
// (X_{-1} = x0), the CoP rows u_k = F_k lambda_k and sum lambda_k = 1.  The polish steps move along the
// null-space basis, so these hold to round-off; its acceptance checks it (SRB_POLISH_EQTOL).
__device__ __forceinline__ double lip_eq_res(const SrbKParams &prm, const double *x0, const double *xs, const double *foot,
                                             int N, int C, int tid, int NTH)
{
    // (x0 and the LDS iterate are read through their own address spaces -- no generic pointer selecting
    // between them: a flat access in this kernel changed its code generation enough to break the polish
    // of the run-time instance)
    double r = 0.0;
#if defined(SRB_DIAG_FLAT_EQRES)         // diagnostic builds only: round 5's first form (one generic pointer)
#ifndef SRB_DIAG_BUILD
#error "SRB_DIAG_FLAT_EQRES is a diagnostic-build option"
#endif
    for (int k = tid; k < N; k += NTH) {
        const double *xp = k ? xs + 4 * (k - 1) : x0;
        const double p0 = xp[0], p1 = xp[1], p2 = xp[2], p3 = xp[3];
#else
    const double g0x = x0[0], g1x = x0[1], g2x = x0[2], g3x = x0[3];
    for (int k = tid; k < N; k += NTH) {
        const int kp = k ? k - 1 : 0;
        const double p0 = k ? xs[4 * kp] : g0x, p1 = k ? xs[4 * kp + 1] : g1x;
        const double p2 = k ? xs[4 * kp + 2] : g2x, p3 = k ? xs[4 * kp + 3] : g3x;
#endif
        const double u0 = xs[4 * N + 2 * k], u1 = xs[4 * N + 2 * k + 1];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const double v = prm.Ad[4 * d] * p0 + prm.Ad[4 * d + 1] * p1 + prm.Ad[4 * d + 2] * p2 +
                             prm.Ad[4 * d + 3] * p3 + prm.Bd[2 * d] * u0 + prm.Bd[2 * d + 1] * u1;
            r = fmax(r, fabs(xs[4 * k + d] - v));
        }
        double g0 = 0.0, g1 = 0.0, sl = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < C) {
                const double lam = xs[6 * N + C * k + j];
                g0 = fma(foot[(2 * k) * C + j], lam, g0); g1 = fma(foot[(2 * k + 1) * C + j], lam, g1); sl += lam;
            }
        r = fmax(r, fmax(fabs(u0 - g0), fmax(fabs(u1 - g1), fabs(sl - 1.0))));
    }
    return r;
}

// Reduced stationarity of the polished point (round 6): g = Z'(grad f(x) + J_A' z_A), grad f from the problem data
// (var_weight, the reference window in LDS) rather than the slots' cost registers, z_A the polish's multipliers
// (ds: active mask, dz: z_A); returns max |M^-1 g| (M: the last Newton step's reduced matrix, Mi its inverse), the
// correction a further step would make, accepted only up to SRB_POLISH_STOL and only where the multipliers that step
// leaves keep their sign (else 1e300).  The other
// tests (feasibility, multiplier signs, converged step, equality rows) held on the points the round-5 generic-
// pointer build returned as OPTIMAL although they were not stationary; this one does not.  The
// term rows are those of the last Newton step (the obstacle rows linearised at its start: O(|dx|) <= 1e-7 off).
// Uniform over the workgroup (every value reduced).  oracle/nlp_ipm.c `polish`: the same test.
template <int NZL, int TS, int NW, int NZE, class TK>
__device__ __forceinline__ double polish_stationary(Slot (&Q)[TS], int nts, const SrbKParams &prm, const double *xs,
                                                  const double *ref, double *CF, double *R, double *OJ, double *zo, int rO,
                                                  int cnt, const ObsFold &OF, int nko, double *vg, double *vy, double *vr,
                                                  double *vd, const double (&Mi)[NZL], const double *H0, int nz, int tid,
                                                  double *part, uint64_t bmask, double *red, int N, int n, int TT, int srow)
{
    SYNC();                                              // every lane's reads of R / OJ / CF / vg of the last step are done
    // the obstacle rows linearised at the polished point itself (the last Newton step, up to 1e-4 when the
    // active rows then hold to 1e-10, ran on rows taken before it: J'z would be off by 2 |dx| |z| there)
    polish_rows<NZL, TS, NW, TK>(Q, nts, xs, OJ, zo, n, rO, R, nz);
    SYNC();
    if constexpr (srb_rhs_slots(TK::compiled, NW, NZL, NZE)) {
        // the coefficients stay in the registers of the lanes that own the slots (rhs_slots): a VEL slot's on the Z row
        // of its variable, a slot of no kind 0 on row 0
        double cfs[TS];
        int rr[TS];
#pragma unroll
        for (int t = 0; t < TS; t++) {
            const Slot &q = Q[t];
            cfs[t] = 0.0; rr[t] = q.r;
            if (t < nts) {
                const double zj = SK_TWO(t) ? q.ds[0] * q.dz[0] - q.ds[1] * q.dz[1] : q.ds[0] * q.dz[0];
                const int kd = SK_KIND(q, t);
                if (SK_EQ(t, kd, K_VAR)) {
                    const int v = q.i0;
                    const double a0 = var_weight(prm, v), gf = fma(a0, xs[v], (v < 4 * N) ? -a0 * ref[v] : 0.0);
                    cfs[t] = gf + zj;
                } else if (SK_EQ(t, kd, K_COP) || SK_EQ(t, kd, K_OBS) || SK_EQ(t, kd, K_VEL)) {
                    cfs[t] = zj;
                }
            }
        }
        rhs_slots<NZL, NZE, TS>(R, cfs, rr, nts, vg, nz, tid & 63);
    } else {
#pragma unroll
    for (int t = 0; t < TS; t++)
        if (t < nts) {
            const Slot &q = Q[t];
            const double zj = SK_TWO(t) ? q.ds[0] * q.dz[0] - q.ds[1] * q.dz[1] : q.ds[0] * q.dz[0];
            const int kd = SK_KIND(q, t);
            if (SK_EQ(t, kd, K_VAR)) {
                const int v = q.i0;
                const double a0 = var_weight(prm, v), gf = fma(a0, xs[v], (v < 4 * N) ? -a0 * ref[v] : 0.0);
                CF[q.wr] = gf + zj;
            } else if (SK_EQ(t, kd, K_COP) || SK_EQ(t, kd, K_OBS)) {
                CF[q.wr] = zj;
            }
        }
    if (NW > 1) SYNC();                                  // the VAR rows' plain stores land before the VEL adds
#pragma unroll
    for (int t = 0; t < TS; t++)
        if (t < nts && SK_IS(Q[t], t, K_VEL))
            __hip_atomic_fetch_add(&CF[Q[t].r], Q[t].ds[0] * Q[t].dz[0] - Q[t].ds[1] * Q[t].dz[1], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
    SYNC();
    rhs_only<NZL, NW>(R, CF, cnt, OF, nko, vg, nz, tid, part, bmask);
    }
    SYNC();
    // the Newton correction g implies, with the last step's inverse (Mi) and matrix (H0): the distance to the
    // stationary point in the reduced coordinates, whatever the scale of the gradient (oracle: the same test)
    double dxs[NZL];
    la_solve<NZL, NW, NZE>(Mi, H0, H0, 0.0, vg, vy, vr, vd, dxs, nz, tid & 63);
    double dm = 0.0;
#pragma unroll
    for (int j = 0; j < NZL; j++) dm = fmax(dm, fabs(dxs[j]));
    // ... and the multipliers that step would leave on the active rows, z_A + rho (c_A + J_A Z dxi) with dxi = -dxs
    // (the polish's own update), must keep their sign: a point stationary only through an active row that
    // should not be active (the row's multiplier of the wrong sign) is not a KKT point either
    constexpr int LDR = NZL + 1;
    double zmin = 1e300, zmax = 1.0;
#pragma unroll
    for (int t = 0; t < TS; t++)
        if (t < nts && (Q[t].ds[0] != 0.0 || (SK_TWO(t) && Q[t].ds[1] != 0.0))) {
            const Slot &q = Q[t];
            const double jd = -((!SRB_OBS_STORED(NZL) && SK_IS(q, t, K_OBS))
                ? fma(OJ[2 * (q.r - rO)], row_dot<NZL, NZE>(R + q.i0 * LDR, dxs),
                      fma(OJ[2 * (q.r - rO) + 1], row_dot<NZL, NZE>(R + q.i1 * LDR, dxs), -row_dot<NZL, NZE>(R + srow * LDR, dxs)))
                : row_dot<NZL, NZE>(R + q.r * LDR, dxs));
#pragma unroll
            for (int r = 0; r < 2; r++)
                if ((SK_TWO(t) || r == 0) && q.ds[r] != 0.0) {
                    const double zn = fma(prm.polish_rho, q.r3[r] + (r ? -jd : jd), q.dz[r]);
                    zmin = fmin(zmin, zn); zmax = fmax(zmax, fabs(zn));
                }
        }
    double rv[2] = {-zmin, zmax};
    wred_x<2, 3u, NW>(rv, red + 5 * 8 * NW, tid);
    // (rho |c_A| <= rho SRB_POLISH_PTOL = 1 is the resolution of that update: the tolerance)
    return (-rv[0] >= -(prm.polish_rho * SRB_POLISH_PTOL + 1e-9 * rv[1])) ? dm : 1e300;
}

// --------------------------------------------------------------------------- shared agent code
// The solve kernel and the polish kernel run on the same per-agent LDS layout and rebuild the
// same null-space basis, so the code they share is written once, as statement macros expanded in
// both template bodies (they bind the locals of the expanding function):
//   SRB_AGENT_LAYOUT     sizes, term-row layout, slot ranges, the LDS carve (srb_lds_doubles)
//   SRB_AGENT_SETUP      inputs (a1/a2/a3: x0, reference window, footholds), Z, xbar, CoM-CoP rows
//   SRB_AGENT_OBSTACLES  the K selected rows per grid (srb_knn_kernel's sel; MPC_dist.cpp:371-396
//                        generalised; neighbours at their planned positions nbr_plan[sel][k], or without a plan
//                        table predicted at constant velocity o_k = p + v Ts (k+1))
//                        (the moving-obstacle instances, MV = 1: static rows at o + w Ts (k+1), w = obs_vel[sel])
//                        (likewise with srb_sizes.obs_eps: the level of static column j is obs_eps[sel[j]])
//                        (and with srb_agent_sizes: neighbour column j at (agent_rad[g] + agent_rad[sel[j]])^2,
//                        every static column at (sqrt(level) + agent_pad[g])^2, g = agent_offset + agent)
//   SRB_AGENT_OUTPUTS    x, the agent's plan (the CoM positions of x), objective, alpha_COM
#define SRB_AGENT_LAYOUT \
    constexpr int NZM = ((NZL + 15) / 16) * 16; \
    constexpr int LDR = NZL + 1, LDH = NZL + 1; \
    constexpr int NTH = 64 * NW; \
    constexpr int NZE = (NC > 0 && CC > 0) ? NC * (CC - 1) + 1 : NZL;   /* reduced size when the shape is compiled */ \
    /* the Gram's vector form (srb_gram.h gram_rhs_vec): one wave, NZL <= 12, stored obstacle rows and the shape compiled in; \
       every other instance keeps gram_rhs (the run-time 12_4_1 and 12_3_1 went deeper into scratch with the vector form) */ \
    constexpr bool GVEC = SRB_GRAM_FORM != SRB_GRAM_MFMA && srb_shape_compiled(NC, CC, KC) && NW == 1 && NZL <= 12 && \
                          SRB_OBS_STORED(NZL) && CC > 1 && NZE <= NZL; \
    using GSH = GramShape<GVEC ? NC : 0, GVEC ? CC : 0, GVEC ? KC : 0>; \
    /* the corrector's right-hand side from slot-owned rows (srb_gram.h rhs_slots): the same instances */ \
    constexpr bool RSL = srb_rhs_slots(srb_shape_compiled(NC, CC, KC), NW, NZL, NZE); \
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6; \
    /* the compiled shape (NC, CC, KC > 0) or the run-time one; n = (6 + C) N + 1, nz = N (C - 1) + 1 */ \
    const int N = NC > 0 ? NC : prm.N, C = CC > 0 ? CC : prm.C, K = KC > 0 ? KC : prm.K_obs + prm.K_nbr; \
    const int n = (NC > 0 && CC > 0) ? (6 + CC) * NC + 1 : prm.n, nz = (NC > 0 && CC > 0) ? NC * (CC - 1) + 1 : prm.nz; \
    const int NK = N * K, NE = 2 * (N - 1); \
    const int n4 = rnd4(n), NK4 = rnd4(NK), UL4 = rnd4(n - 4 * N); \
    const int E4 = (4 * N + NE + 16 * NW - 1) / (16 * NW) * (16 * NW) - 4 * N;   /* CoM-CoP block: rU a multiple of 16 NW */ \
    /* stored term rows: X (4N) | CoM-CoP (E4) | U, lambda, slack (UL4) | zero rows up to rO, a */ \
    /* multiple of 16 NW; then the NKP (NK padded likewise) generated obstacle terms: TT terms */ \
    const int rC = 4 * N, rU = rC + E4, rO = (rU + UL4 + 16 * NW - 1) / (16 * NW) * (16 * NW); \
    const int NKP = (NK + 16 * NW - 1) / (16 * NW) * (16 * NW), TT = rO + NKP; \
    const TermLayout TL{N, C, n, nz, E4}; \
    const uint64_t bmask = full_batches<NZM>(rO, N, C, n, rC, NE, rU, lane);   /* stored-row batches needing every column block */ \
    const int NOP = (3 * N + 16 * NW - 1) / (16 * NW) * (16 * NW);   /* folded obstacle grid terms (3 a grid), padded */ \
    const int sE = n, sV = n + NE, sO = sV + 2 * N, S = sO + NK; \
    const double tol = prm.tol, th = tol / sqrt(3.0); \
    STAMP_DECL; \
    /* LDS carve (must match srb_lds_doubles) */ \
    double *p = lds; \
    double *R = p; p += (SRB_OBS_STORED(NZL) ? TT : rO) * LDR;   /* stored term rows (Z rows first; + obstacle rows) */ \
    double *W = p; p += TT + 1;                   /* gram weights (+ one scratch entry) */ \
    double *CF = p; p += TT + 1;                  /* rhs coefficients (+ one scratch entry) */ \
    double *OJ = p; p += SRB_OBS_STORED(NZL) ? 0 : 2 * NKP;       /* folded instances: obstacle rows' jx, jy */ \
    double *FO = p; p += SRB_OBS_STORED(NZL) ? 0 : 9 * (N + 1);   /* per-grid obstacle fold S_k, c_k (+ a zero grid) */ \
    const ObsFold OF{OJ, FO, rO, N, K, NOP, full_obs_batches<NZM>(N, C, NOP, lane), rU, C, n}; \
    double *H0 = p; p += NZL * LDH;               /* assembled Z'HZ (unshifted; + delta Z'Z on the fly) */ \
    double *ZZ = p; p += NZL * LDH;               /* Z'Z (NLP) */ \
    double *vg = p; p += NZM; double *vy = p; p += NZM; double *vr = p; p += NZM; double *vd = p; p += NZM; \
    double *xs = p; p += n4; \
    double *xb = p; p += n4;                      /* xbar (setup); then dx = Z dxi of the Newton steps (dxv) */ \
    double *dxv = xb; \
    double *xsv = p; p += n4;                     /* NLP: saved iterate (round-off floor / polish) */ \
    double *xprev = p; p += n4;                   /* the iterate before the last update (non-finite fallback) */ \
    double *ref = p; p += 4 * N; \
    double *foot = p; p += 2 * C * N; \
    double *obs = SRB_OBS_IN_ZZ(NZL, NK) ? ZZ : p; p += SRB_OBS_IN_ZZ(NZL, NK) ? 0 : 2 * NK + 2;   /* obstacle positions (setup) */ \
    double *eps = p; p += K + 1; \
    double *zo = p; p += NK4;                     /* obstacle duals (per-grid sums) */ \
    int *sel = (int *)p; p += (K + 1); \
    double *red = p; p += (NW > 1) ? 8 * SRB_RED_SITES * NW : 0;   /* cross-wave reduction sites */ \
    double *part = p; p += (NW > 2) ? NW * ((NZM == 16) ? 1 : 3) * 256 + NW * NZM : 0;   /* partial Gram / rhs (NW = 4) */ \
    float *zpl = (float *)p; p += SRB_FUSED_POLISH_OK(NZL) ? rnd4(S) : 0;   /* fused polish: the exported active set (2 floats a slot) */ \
    const int RROWS = SRB_OBS_STORED(NZL) ? TT : rO;   /* term rows stored in R */ \
    LCK_INIT(); \
    LCK((int)(p - lds) <= srb_lds_doubles(prm, NZL, NW), 0); \
    LCK(rU <= RROWS && (!SRB_OBS_STORED(NZL) || rO + NKP <= TT), 4); \
    (void)RROWS; \
    do {} while (0)

#define SRB_AGENT_SETUP \
    const double *x0 = x0g + 4 * (size_t)agent; \
    for (int i = tid; i < 4 * N; i += NTH) ref[i] = refg[(size_t)agent * 4 * N + i]; \
    for (int i = tid; i < 2 * C * N; i += NTH) foot[i] = footg[(size_t)agent * 2 * C * N + i]; \
    if (prm.use_nlp && tid < K) sel[tid] = sel_g[(size_t)agent * K + tid]; \
    for (int i = tid; i < (int)(xs - R) + 2 * n4; i += NTH) R[i] = 0.0; \
    for (int i = tid; i < NK4; i += NTH) zo[i] = 0.0; \
    SYNC(); \
    STAMP_END(23);                 /* stamps build: inputs loaded, LDS cleared */ \
    if (prm.use_nlp) { SRB_AGENT_OBSTACLES; } \
    STAMP_END(24);                 /* stamps build: obstacle rows */ \
    /* null-space basis Z and particular point xbar (forward LIP rollout, MPC_dist.cpp:232-261) */ \
    if (tid == 0) { \
        double X[4] = {x0[0], x0[1], x0[2], x0[3]}; \
        for (int k = 0; k < N; k++) { \
            const double u0 = foot[(k * 2 + 0) * C + C - 1], u1 = foot[(k * 2 + 1) * C + C - 1]; \
            double Xn[4]; \
            for (int d = 0; d < 4; d++) \
                Xn[d] = prm.Ad[d * 4] * X[0] + prm.Ad[d * 4 + 1] * X[1] + prm.Ad[d * 4 + 2] * X[2] + prm.Ad[d * 4 + 3] * X[3] + \
                        prm.Bd[d * 2] * u0 + prm.Bd[d * 2 + 1] * u1; \
            for (int d = 0; d < 4; d++) { X[d] = Xn[d]; xb[4 * k + d] = Xn[d]; } \
            xb[4 * N + 2 * k] = u0; xb[4 * N + 2 * k + 1] = u1; \
            for (int j = 0; j < C; j++) xb[6 * N + C * k + j] = (j == C - 1) ? 1.0 : 0.0; \
        } \
        xb[n - 1] = 0.0; \
    } \
    for (int cg = tid; cg < nz - 1; cg += NTH) {   /* column 1 + cg: dof t of grid j (column 0: the slack) */ \
        const int j = cg / (C - 1), t = cg % (C - 1), col = cg + 1; \
        double lam[4]; \
        const int is_null = lambda_basis(foot + j * 2 * C, C, t, lam); \
        double g0 = 0.0, g1 = 0.0; \
        if (!is_null) \
            _Pragma("unroll") for (int i = 0; i < 4; i++) \
                if (i < C) { g0 += foot[(j * 2 + 0) * C + i] * lam[i]; g1 += foot[(j * 2 + 1) * C + i] * lam[i]; } \
        _Pragma("unroll") for (int i = 0; i < 4; i++) if (i < C) R[TL.zr(6 * N + C * j + i) * LDR + col] = lam[i]; \
        R[TL.zr(4 * N + 2 * j) * LDR + col] = g0; \
        R[TL.zr(4 * N + 2 * j + 1) * LDR + col] = g1; \
        double v[4]; \
        for (int d = 0; d < 4; d++) v[d] = prm.Bd[d * 2] * g0 + prm.Bd[d * 2 + 1] * g1; \
        for (int k = j; k < N; k++) { \
            for (int d = 0; d < 4; d++) R[(4 * k + d) * LDR + col] = v[d]; \
            double tt[4]; \
            for (int d = 0; d < 4; d++) tt[d] = prm.Ad[d * 4] * v[0] + prm.Ad[d * 4 + 1] * v[1] + prm.Ad[d * 4 + 2] * v[2] + prm.Ad[d * 4 + 3] * v[3]; \
            for (int d = 0; d < 4; d++) v[d] = tt[d]; \
        } \
    } \
    if (tid == 0) R[TL.zr(n - 1) * LDR] = 1.0; \
    SYNC(); \
    STAMP_END(25);                 /* stamps build: null-space basis, xbar */ \
    /* CoM-CoP term rows M_e = Z_p - Z_u (p: CoM of grid i, u: CoP of grid i+1); xs = xbar */ \
    if (tid < NE) { \
        const int i = tid >> 1, d = tid & 1, pp = 4 * i + 2 * d, uu = 4 * N + 2 * (i + 1) + d; \
        for (int a = 0; a < NZL; a++) Rt[tid * LDR + a] = R[pp * LDR + a] - R[TL.zr(uu) * LDR + a]; \
    } \
    for (int v = tid; v < n; v += NTH) xs[v] = xb[v]; \
    do {} while (0)

#define SRB_AGENT_OBSTACLES \
    /* every (grid k, row j) pair on its own lane, all loads of a lane issued before its stores */ \
    { \
        double ox_[TS], oy_[TS]; \
        _Pragma("unroll") for (int t = 0; t < TS; t++) { \
            const int e = tid + NTH * t; \
            ox_[t] = oy_[t] = 0.0; \
            if (e < NK) { \
                const int k = e / K, j = e - k * K; \
                const bool st = j < prm.K_obs; \
                const int bi = sel[j]; \
                const double tt = st ? 0.0 : prm.Ts * (k + 1); \
                const size_t bj = (bi >= 0) ? bi : 0; \
                if (nbr_plan) {   /* a kernel argument: the branch is wave-uniform */ \
                    /* neighbour rows from the plan table: row sel[j], grid k is that agent's (x, y) at Ts (k + 1) */ \
                    const double *srcp = st ? obstacles + 2 * bj : nbr_plan + 2 * (bj * (size_t)N + k); \
                    ox_[t] = (bi >= 0) ? srcp[0] : x0[0] + 1000.0; \
                    oy_[t] = (bi >= 0) ? srcp[1] : x0[2]; \
                } else { \
                    const double *srcp = st ? obstacles + 2 * bj : nbr_state + 4 * bj; \
                    /* no selection (-1): a row 1000 m along +x, as the oracle */ \
                    ox_[t] = (bi >= 0) ? srcp[0] + (st ? 0.0 : srcp[2] * tt) : x0[0] + 1000.0; \
                    oy_[t] = (bi >= 0) ? srcp[1] + (st ? 0.0 : srcp[3] * tt) : x0[2]; \
                } \
                if (MV && obs_vel) {   /* MV: the moving-obstacle instances only; a kernel argument: wave-uniform */ \
                    /* moving obstacles: the static row sel[j] at grid k is o + w (Ts (k + 1)), w = obs_vel[sel[j]], */ \
                    /* uncontracted (the bits srb_knn_obs_horizon_kernel scans); the -1 row and the neighbour rows */ \
                    /* are those of the arms above, with or without a plan table */ \
                    _Pragma("clang fp contract(off)") \
                    if (st && bi >= 0) { \
                        const double tk = prm.Ts * (k + 1); \
                        ox_[t] = obstacles[2 * bj] + obs_vel[2 * bj] * tk; \
                        oy_[t] = obstacles[2 * bj + 1] + obs_vel[2 * bj + 1] * tk; \
                    } \
                } \
            } \
        } \
        _Pragma("unroll") for (int t = 0; t < TS; t++) { \
            const int e = tid + NTH * t; \
            if (e < NK) { obs[2 * e] = ox_[t]; obs[2 * e + 1] = oy_[t]; } \
        } \
        if (tid < K) eps[tid] = (tid < prm.K_obs) ? prm.eps_obs : prm.eps_nbr; \
        /* obstacle sizes (srb_sizes.obs_eps; the MV instances only, a kernel argument: wave-uniform): the level of */ \
        /* static column j is the table's row sel[j]; the lane that wrote the entry rewrites it (no barrier added); */ \
        /* the neighbour columns and a -1 row keep what they have */ \
        if (MV && obs_eps) { if (tid < prm.K_obs && sel[tid] >= 0) eps[tid] = obs_eps[sel[tid]]; } \
        /* agent sizes (srb_agent_sizes; the MV instances only, kernel arguments: wave-uniform), rad then pad, each */ \
        /* lane again on the entry it wrote itself.  rad: the level of neighbour column j is the squared sum of the */ \
        /* agent's own safety radius (table row agent_offset + agent) and the neighbour's (row sel[j]), a -1 row */ \
        /* keeps eps_nbr.  pad: every static column's safety radius sqrt(level) grows by the agent's own pad. */ \
        /* One rounded operation each: uncontracted, the bits of the host restatement */ \
        if (MV && agent_rad) { \
            _Pragma("clang fp contract(off)") \
            if (tid >= prm.K_obs && tid < K && sel[tid] >= 0) { \
                const double s_ = agent_rad[(size_t)agent_offset + agent] + agent_rad[sel[tid]]; \
                eps[tid] = s_ * s_; \
            } \
        } \
        if (MV && agent_pad) { \
            _Pragma("clang fp contract(off)") \
            if (tid < prm.K_obs) { \
                const double t_ = sqrt(eps[tid]) + agent_pad[(size_t)agent_offset + agent]; \
                eps[tid] = t_ * t_; \
            } \
        } \
    } \
    do {} while (0)

#define SRB_AGENT_OUTPUTS \
    /* x and the objective 0.5 x'Q_qp x + f'x (ExCost::GetCost, dec_vars_constr_cost.h:423-438) */ \
    double f = 0.0; \
    for (int v = tid; v < n; v += NTH) { \
        const double xv = xs[v]; \
        x_out[(size_t)agent * n + v] = xv; \
        /* the plan: (x, y) of grid k = x[4k], x[4k + 2], the even entries of X */ \
        if (plan_out && v < 4 * N && !(v & 1)) plan_out[(size_t)agent * 2 * N + (v >> 1)] = xv; \
        const double a0 = var_weight(prm, v), a1 = (v < 4 * N) ? -a0 * ref[v] : 0.0; \
        f += fma(0.5 * a0 * xv, xv, a1 * xv); \
    } \
    { \
        double rv[1] = {f}; \
        wred_x<1, 0u, NW>(rv, red + 6 * 8 * NW, tid); \
        f = rv[0]; \
    } \
    /* fitComTrajectory_eventbase (MPC_dist.cpp:784-855) as an epilogue: alpha_COM (4 x 5) interpolates */ \
    /* [buffer, X_0..X_3] at s = 0, 1/4, .., 1 (the reference's 24 x 24 KKT keeps only the s = 0 end */ \
    /* point row, so its solution is this interpolation): alpha[d][j] = sum_i Binv[j][i] p_i[d] */ \
    if (alpha_out && tid < 20) { \
        const int d = tid / 5, j = tid - 5 * (tid / 5); \
        double acc = prm.Binv[5 * j] * alpha_buf[(size_t)agent * 4 + d]; \
        for (int i = 1; i < 5; i++) acc = fma(prm.Binv[5 * j + i], xs[4 * (i - 1) + d], acc); \
        alpha_out[(size_t)agent * 20 + 5 * d + j] = acc; \
    } \
    do {} while (0)

// Diagnostic builds only (-DSRB_DIAG_POLISH_OUT, make lipvar): the fused polish's last acceptance test --
// its stationarity ratio (or, where the other tests failed, its equality residual) into obj, the tests it met
// as bits into the QP iteration count (1 primal, 2 active rows, 4 multipliers, 8 last step, 16 equality rows,
// 32 equality residual not finite, 64 a pass ran, 128 stationary)
#ifdef SRB_DIAG_POLISH_OUT
#ifndef SRB_DIAG_BUILD
#error "SRB_DIAG_POLISH_OUT is a diagnostic-build option"
#endif
#define SRB_POLISH_DIAG() do { dg_eqr = pcand ? sratio : eqr; dg_bits = 64 | (pv <= SRB_POLISH_PTOL) | ((cv <= SRB_POLISH_PTOL) << 1) | \
    ((nzmin <= 1e-9 * zm) << 2) | ((lastdx <= SRB_POLISH_DXTOL) << 3) | ((eqr <= SRB_POLISH_EQTOL) << 4) | ((!isfinite(eqr)) << 5) | \
    ((pcand && sratio <= SRB_POLISH_STOL) << 7); } while (0)
#else
#define SRB_POLISH_DIAG() do {} while (0)
#endif

// The passes of the active-set polish (polish_agent, and the fused polish at the end of nmpc_agent):
// PS[t] holds each slot's active mask (ds), multiplier z_A (dz) and the inactive rows' proximal weight
// (s); xs the interior-point result, also saved in xsv.  Sets `accepted`.
#define SRB_POLISH_PASSES_LOOP(PS)                                                                                                            \
_Pragma("clang loop unroll(disable)")                                                                                                         \
    for (int pass = 0; pass < SRB_POLISH_PASSES; pass++) {                                                                                    \
        bool bad = false;                                                                                                                     \
        double lastdx = 1e300;                                                                                                                \
_Pragma("clang loop unroll(disable)")                                                                                                         \
        for (int pit = 0; pit < SRB_POLISH_IT; pit++) {                                                                                       \
            SYNC(); /* xs of the previous step / pass */                                                                                      \
            polish_rows<NZL, TS, NW, TK>(PS, nts, xs, OJ, zo, n, rO, R, nz); /* q.jd = g(x), M_o (OJ), zo = z_A */                            \
            SYNC(); /* R rows, zo */                                                                                                          \
            if (pit > 0) { /* converged after a small step (oracle, same rule) */                                                             \
                double cm = 0.0;                                                                                                              \
_Pragma("unroll")                                                                                                                             \
                for (int t = 0; t < TS; t++)                                                                                                  \
                    if (t < nts) {                                                                                                            \
                        const Slot &q = PS[t];                                                                                                \
                        if (SK_TWO(t)) cm = fmax(cm, fmax(q.ds[0] * fabs(q.jd - q.h[0]), q.ds[1] * fabs(q.jd + q.h[1])));                    \
                        else cm = fmax(cm, fmax(q.ds[0] * fabs(q.jd - q.h[0]), 0.0)); /* (single-row trip: row 1 is off) */                   \
                    }                                                                                                                         \
                double rv[1] = {cm};                                                                                                          \
                wred_x<1, 1u, NW>(rv, red + 6 * 8 * NW, tid);                                                                                 \
                if (lastdx <= SRB_POLISH_DX1 && rv[0] <= SRB_POLISH_CTOL) { lastdx = 0.0; break; }                                            \
            }                                                                                                                                 \
_Pragma("unroll")                                                                                                                             \
            for (int t = 0; t < TS; t++)                                                                                                      \
                if (t < nts) {                                                                                                                \
                    Slot &q = PS[t];                                                                                                          \
                    q.r3[0] = q.jd - q.h[0];                                                                                                  \
                    if (SK_TWO(t)) q.r3[1] = -q.jd - q.h[1];                                                                                 \
                    const double cfa = SK_TWO(t)                                                                                              \
                        ? q.ds[0] * fma(prm.polish_rho, q.r3[0], q.dz[0]) - q.ds[1] * fma(prm.polish_rho, q.r3[1], q.dz[1])                   \
                        : q.ds[0] * fma(prm.polish_rho, q.r3[0], q.dz[0]);                                                                    \
                    const double wa = SK_TWO(t) ? (q.ds[0] != 0.0 ? prm.polish_rho : q.s[0]) + (q.ds[1] != 0.0 ? prm.polish_rho : q.s[1])     \
                                                : (q.ds[0] != 0.0 ? prm.polish_rho : q.s[0]);                                                 \
                    if (SK_IS(q, t, K_VAR)) {                                                                                             \
                        double hs = 0.0;                                                                                                      \
                        if (SK_COM(t) && q.i0 < 4 * N && !(q.i0 & 1)) hs = -2.0 * zo_sum(zo, q.i0 >> 2, K);                                           \
                        W[q.wr] = q.a0 + hs + wa;                                                                                             \
                        CF[q.wr] = -(fma(q.a0, q.jd, q.a1) + cfa);                                                                            \
                    } else {                                                                                                                  \
                        W[q.wr] = wa; /* COP / OBS rows (VEL: the scratch entry) */                                                           \
                        CF[q.wr] = -cfa;                                                                                                      \
                    }                                                                                                                         \
                }                                                                                                                             \
            if (NW > 1) SYNC(); /* the VAR rows' plain stores land before the VEL adds */                                                     \
_Pragma("unroll")                                                                                                                             \
            for (int t = 0; t < TS; t++)                                                                                                      \
                if (t < nts && SK_IS(PS[t], t, K_VEL)) {                                                                                     \
                    const Slot &q = PS[t];                                                                                                    \
                    const double cfa = q.ds[0] * fma(prm.polish_rho, q.r3[0], q.dz[0]) - q.ds[1] * fma(prm.polish_rho, q.r3[1], q.dz[1]);     \
                    __hip_atomic_fetch_add(&W[q.r], (q.ds[0] != 0.0 ? prm.polish_rho : q.s[0]) + (q.ds[1] != 0.0 ? prm.polish_rho : q.s[1]),  \
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);                                                   \
                    __hip_atomic_fetch_add(&CF[q.r], -cfa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);                                   \
                }                                                                                                                             \
            SYNC();                                                                                                                           \
            if constexpr (GVEC) gram_rhs_vec<NZL, true, GSH, SRB_GRAM_FORM>(R, W, CF, OF, nko, H0, vg, nz, lane); else gram_rhs<NZL, true, NW>(R, W, CF, cnt, OF, nko, H0, vg, nz, tid, part, bmask);                                                    \
            SYNC();                                                                                                                           \
            if (pass == 0 && pit == 0) POLDBG_MAT(H0, LDH, vg, nz);                                                                           \
            gj_load<NZL, NZE>(Mi, H0, ZZ, 0.0, nz, lane);                                                                                          \
            if (gj_factor<NZL, NZE>(Mi, nz, lane, 0) != 0) { bad = true; break; } /* not PD: reject */                                            \
            la_solve<NZL, NW, NZE>(Mi, H0, ZZ, 0.0, vg, vy, vr, vd, dxi, nz, lane);                                                                    \
            double mdx = 0.0;                                                                                                                 \
_Pragma("unroll")                                                                                                                             \
            for (int t = 0; t < TS; t++)                                                                                                      \
                if (t < nts) {                                                                                                                \
                    Slot &q = PS[t];                                                                                                          \
                    const double jd = (!SRB_OBS_STORED(NZL) && SK_IS(q, t, K_OBS)) /* J_o Z dxi, folded instances (OJ) */                \
                        ? fma(OJ[2 * (q.r - rO)], row_dot<NZL, NZE>(R + q.i0 * LDR, dxi),                                                          \
                              fma(OJ[2 * (q.r - rO) + 1], row_dot<NZL, NZE>(R + q.i1 * LDR, dxi), -row_dot<NZL, NZE>(R + TL.zr(n - 1) * LDR, dxi)))     \
                        : row_dot<NZL, NZE>(R + q.r * LDR, dxi);                                                                                   \
                    q.dz[0] = fma(q.ds[0] * prm.polish_rho, q.r3[0] + jd, q.dz[0]);                                                           \
                    if (SK_TWO(t)) q.dz[1] = fma(q.ds[1] * prm.polish_rho, q.r3[1] - jd, q.dz[1]);                                                      \
                    if (SK_IS(q, t, K_VAR)) {                                                                                                \
                        xs[q.i0] = q.jd + jd; /* every read of xs this step is behind a barrier */                                            \
                        mdx = fmax(mdx, fabs(jd));                                                                                            \
                    }                                                                                                                         \
                }                                                                                                                             \
            {                                                                                                                                 \
                double rv[1] = {mdx};                                                                                                         \
                wred_x<1, 1u, NW>(rv, red + 8 * 8 * NW, tid);                                                                                 \
                lastdx = rv[0];                                                                                                               \
            }                                                                                                                                 \
            POLDBG(4 + pass, pit, lastdx);                                                                                                    \
            POLDBG_X(pass, pit, xs, n);                                                                                                       \
            if (lastdx <= SRB_POLISH_DXTOL) break; /* converged: no further step */                                                           \
        }                                                                                                                                     \
        if (bad) break;                                                                                                                       \
        SYNC();                                                                                                                               \
 /* ---- acceptance at the polished point */                                                                                                  \
        double pv = -1e300, cv = 0.0, nzmin = -1e300, zm = 1.0, vi = -1e300, eqr = 0.0;                                                       \
        {                                                                                                                                     \
            const double s_var = xs[n - 1];                                                                                                   \
_Pragma("unroll")                                                                                                                             \
            for (int t = 0; t < TS; t++)                                                                                                      \
                if (t < nts) {                                                                                                                \
                    Slot &q = PS[t];                                                                                                          \
                    const double fq = slot_f<TK>(q, t, xs, s_var);                                                                            \
_Pragma("unroll")                                                                                                                             \
                    for (int r = 0; r < 2; r++)                                                                                               \
                        if (SK_TWO(t) || r == 0) {                                                                                           \
                            const double v = r ? -fq - q.h[1] : fq - q.h[0];                                                                  \
                            q.r3[r] = v;                                                                                                      \
                            if (SK_M(q, t, r) != 0.0) pv = fmax(pv, v);                                                                      \
                            if (q.ds[r] != 0.0) { cv = fmax(cv, fabs(v)); nzmin = fmax(nzmin, -q.dz[r]); zm = fmax(zm, fabs(q.dz[r])); }      \
                            else if (SK_M(q, t, r) != 0.0) vi = fmax(vi, v);                                                                 \
                        }                                                                                                                     \
                }                                                                                                                             \
            double rv[6] = {pv, cv, nzmin, zm, vi, lip_eq_res(prm, x0, xs, foot, N, C, tid, NTH)};                                   \
            wred_x<6, 0x3Fu, NW>(rv, red + 7 * 8 * NW, tid);                                                                                  \
            pv = rv[0]; cv = rv[1]; nzmin = rv[2]; zm = rv[3]; vi = rv[4]; eqr = rv[5];                                                       \
        }                                                                                                                                     \
        POLDBG(pass, 0, pv); POLDBG(pass, 1, cv); POLDBG(pass, 2, nzmin); POLDBG(pass, 3, zm); POLDBG(pass, 4, vi);                           \
        POLDBG(pass, 5, lastdx); POLDBG(pass, 7, eqr);                                                                                        \
        const bool pcand = pv <= SRB_POLISH_PTOL && cv <= SRB_POLISH_PTOL && nzmin <= 1e-9 * zm && lastdx <= SRB_POLISH_DXTOL &&           \
                           eqr <= SRB_POLISH_EQTOL;                                                                                           \
        const double sratio = pcand ? polish_stationary<NZL, TS, NW, NZE, TK>(PS, nts, prm, xs, ref, CF, R, OJ, zo, rO, cnt, OF, nko, vg, vy,\
                                                              vr, vd, Mi, H0, nz, tid, part, bmask, red, N, n, TT, TL.zr(n - 1)) : 0.0;       \
        SRB_POLISH_DIAG();                                                                                                                    \
        if (pcand && sratio <= SRB_POLISH_STOL) {                                                                                             \
            POLDBG(pass, 6, 1.0);                                                                                                             \
            accepted = true;                                                                                                                  \
            break;                                                                                                                            \
        }                                                                                                                                     \
 /* next pass: the most negative multiplier leaves A, violated rows join; the rows */                                                         \
 /* that stay keep their multipliers (>= 0), the new ones start at 0 */                                                                       \
        double wd = 1e300;                                                                                                                    \
        int wk = 0x7fffffff;                                                                                                                  \
_Pragma("unroll")                                                                                                                             \
        for (int t = 0; t < TS; t++)                                                                                                          \
            if (t < nts)                                                                                                                      \
_Pragma("unroll")                                                                                                                             \
                for (int r = 0; r < 2; r++)                                                                                                   \
                    if ((SK_TWO(t) || r == 0) && PS[t].ds[r] != 0.0 && PS[t].dz[r] < -1e-9 * zm) lexmin(wd, wk, PS[t].dz[r], 2 * (tid + NTH * t) + r);                 \
        wargmin_x<NW>(wd, wk, red + 9 * 8 * NW, tid);                                                                                         \
        if (wk == 0x7fffffff && !(vi > SRB_POLISH_PTOL)) break; /* nothing to change: rejected */                                             \
_Pragma("unroll")                                                                                                                             \
        for (int t = 0; t < TS; t++) {                                                                                                        \
            Slot &q = PS[t];                                                                                                                  \
_Pragma("unroll")                                                                                                                             \
            for (int r = 0; r < 2; r++)                                                                                                       \
                if (SK_TWO(t) || r == 0) {                                                                                                   \
                    if (2 * (tid + NTH * t) + r == wk) q.ds[r] = 0.0;                                                                         \
                    else if (t < nts && q.ds[r] == 0.0 && SK_M(q, t, r) != 0.0 && q.r3[r] > SRB_POLISH_PTOL) q.ds[r] = 1.0;                  \
                    q.dz[r] = q.ds[r] * fmax(q.dz[r], 0.0);                                                                                   \
                }                                                                                                                             \
        }                                                                                                                                     \
        SYNC();                                                                                                                               \
        for (int v = tid; v < n; v += NTH) xs[v] = xsv[v]; /* the next pass starts from the interior-point result */                          \
    }                                                                                                                                         \
    do {} while (0)

// a + b as a sum of its own, never contracted with a product that formed b.  The split stage bodies' set_rhs adds the
// centring term sigma mu with it: in the NLP's own copy that term is a plain product (pc is a constant there), and
// fused into the sum it would round differently from the one body of both stages, where a select stands between
__device__ __forceinline__ double add_plain(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

// --------------------------------------------------------------------------- main kernel
// NZL: register bound on nz (one reduced-matrix row per lane); TS: slot trips per thread;
// NW: wavefronts per agent (1, or 4 = one per SIMD of a CU for small batches).  With NW > 1
// the row slots and the term-row passes are split across the waves and combined through LDS;
// the reduced-system factorisation and solves run redundantly in every wave (identical data,
// identical results, no communication).
template <int NZL, int TS, int NW, int NC, int CC, int KC, int KF = 0, int MV = 0>
__device__ __forceinline__ void nmpc_agent(const SrbKParams &prm, int agent,
                const double *__restrict__ x0g, const double *__restrict__ refg, const double *__restrict__ footg,
                const double *__restrict__ obstacles, int n_obs,
                const double *__restrict__ nbr_state, int n_all, int agent_offset,
                double *__restrict__ x_qp_out, double *__restrict__ x_out,
                double *__restrict__ obj_out, int *__restrict__ status_out, int *__restrict__ iters_out,
                const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,
                const int *__restrict__ sel_g, float *__restrict__ zpol_g, int zstride,
                const double *__restrict__ nbr_plan, double *__restrict__ plan_out,
                const double *__restrict__ obs_vel, const double *__restrict__ obs_eps,
                const double *__restrict__ agent_rad, const double *__restrict__ agent_pad, double *lds)
{
    SRB_AGENT_LAYOUT;
#ifdef SRB_STAMPS
    unsigned long long *stamp_lds = (unsigned long long *)p; p += SRB_NSTAMP;
    if (tid < 64) stamp_lds[tid] = 0;
#endif
    double *Rt = R + rC * LDR;                          // CoM-CoP rows
    using TK = SlotTrips<NTH, TS, NC, CC, KC>;          // the kinds each slot trip can hold (compiled shapes)

    STAMP_BEGIN();
    // ---- inputs (a1/a2/a3: x0, reference window, footholds), null-space basis Z, xbar, term rows
    SRB_AGENT_SETUP;

    // ---- slot constants
    Slot Q[TS];
#pragma unroll
    for (int t = 0; t < TS; t++) {
        slot_init(Q[t], tid + NTH * t, prm, TL, ref, sE, sV, sO, S, rC, rO, K, TT);
        SRB_SLOT_LCK(Q[t], tid + NTH * t);
    }
    double Mi[NZL];                                          // inverse of the reduced Newton matrix (row = lane)
    double dxi[NZL];                                         // Newton direction in xi (uniform)
#pragma unroll
    for (int j = 0; j < NZL; j++) { Mi[j] = (mrow<NZL>(lane) == j) ? 1.0 : 0.0; dxi[j] = 0.0; }
    // LEAN (the N = 20 instances, NZL 24): 1/z, 1/s, dsT and r3 are recomputed where they are used
    // instead of held per slot across the Newton solve (16 VGPRs a slot, 64 at TS = 4: the loop's
    // spills); the same expressions in the same order, so the results are bit-identical
    constexpr bool LEAN = NZL > 16;
    auto IZ = [&](const Slot &q, int r) -> double { if constexpr (LEAN) return rcp_d(q.z[r]); else return q.iz[r]; };
    auto IS = [&](const Slot &q, int r) -> double { if constexpr (LEAN) return rcp_d(q.s[r]); else return q.is[r]; };
    SYNC();
    STAMP_END(0);

    int qp_flag = 3, qp_it = 0, nlp_flag = 0, nlp_it = 0;
#ifdef SRB_DIAG_POLISH_OUT
    double dg_eqr = -1.0;
    int dg_bits = 0;
#endif
    const int nstage = prm.use_nlp ? 2 : 1;
    // The stage body (srb_stage_body.h) is compiled once per stage where that pays and once for both elsewhere.
    // SPLIT, the compiled shapes with one column block (12_4_1_10_2_11, 12_1_4_10_2_3, their f32 and mv forms): a copy
    // with nl a compile-time false and one with true, so the QP copy holds nothing of the NLP's (obstacle terms, the
    // 14-try shift loop, the near / save / restore logic) and in both the slot trips, row masks and obstacle range
    // fold.  Their wave time is instruction issue and the instruction cache is no limiter there (5.4 misses a wave,
    // DESIGN.md section 6), so the larger code object costs nothing that the kernel waits for.
    // Every other instance keeps one loop over the two stages, the iteration once in the code object: the run-time
    // shapes are heavily spilled already (12_4_1_0_0_0: 304 B of scratch a lane) and that instance with two bodies
    // returned wrong results at N = 11 for a reason not found; two bodies put the NZL 24 compiled instance
    // 24_4_2_20_2_11 into scratch.
    // The body is textually included, not called: a lambda over the function's state changed the machine code of
    // the run-time instances and broke N = 11 and N = 12.
    constexpr bool SPLIT = TK::compiled && NZL <= 16;
    if constexpr (SPLIT) {
        do {
            constexpr int stage = 0;
            constexpr bool nl = false;
#include "srb_stage_body.h"
        } while (0);
        if (nstage == 2)
            do {
                constexpr int stage = 1;
                constexpr bool nl = true;
#include "srb_stage_body.h"
            } while (0);
    } else {
#pragma clang loop unroll(disable)
        for (int stage = 0; stage < nstage; stage++) {
            const bool nl = stage == 1;
#include "srb_stage_body.h"
        }
    }
    SYNC();
    if (x_qp_out && nstage == 1)
        for (int v = tid; v < n; v += NTH) x_qp_out[(size_t)agent * n + v] = xs[v];
    // ---- fused active-set polish (prm.polish_fused; otherwise srb_polish_kernel runs next): the same
    // passes on the LDS state the NLP stage left (term rows, iterate) with the interior-point slots
    // reused as the polish's (their state is dead here), so an agent that finishes early polishes on
    // its own SIMD while slower agents still iterate, and nothing goes through HBM.  Compiled for the
    // instances up to SRB_FUSED_POLISH_MAX (NZL 24 since round 5: N = 20 included, 28 B of scratch per lane
    // in 24_4_2_20_2_11, config 5 2.49 -> 2.12 ms with the compiled horizon; NZL 32 keeps the kernel)
    if constexpr (SRB_FUSED_POLISH_OK(NZL))
    if (prm.polish_fused && prm.use_nlp && nlp_flag != 1 && nlp_flag != 3) {
        const int nts = (S + NTH - 1) / NTH;
        const int cnt = rU, nko = NKP;
        for (int v = tid; v < n; v += NTH) xsv[v] = xs[v];
#pragma unroll
        for (int t = 0; t < TS; t++) {
            const int sl = tid + NTH * t;
#pragma unroll
            for (int r = 0; r < 2; r++)
            if (SK_TWO(t) || r == 0) {
                LCK(!(t < nts && sl < S) || 2 * sl + r < 2 * rnd4(S), 6);
                const double v = (t < nts && sl < S) ? (double)zpl[2 * sl + r] : 0.0;
                Q[t].ds[r] = (v > 0.0) ? 1.0 : 0.0;
                Q[t].dz[r] = fmax(v, 0.0);
                Q[t].s[r] = fmax(-v, 0.0);
            }
        }
        bool accepted = false;
#ifdef SRB_DIAG_CORRUPT_COST       // diagnostic builds only: the defect class of the round-5 generic-pointer build --
#ifndef SRB_DIAG_BUILD             // the polish's cost registers off (here c_v of the X rows by 1 %), its data intact
#error "SRB_DIAG_CORRUPT_COST is a diagnostic-build option"
#endif
#pragma unroll
        for (int t = 0; t < TS; t++)
            if (Q[t].kind == K_VAR && Q[t].i0 < 4 * N) Q[t].a1 *= 1.01;
#endif
        SRB_POLISH_PASSES_LOOP(Q);
        SYNC();
        if (accepted) nlp_flag = 0;
        else
            for (int v = tid; v < n; v += NTH) xs[v] = xsv[v];
        SYNC();
        STAMP_END(26);                                      // stamps build: the fused polish
    }

    // ---- outputs: x, objective (ExCost::GetCost, dec_vars_constr_cost.h:423-438), alpha_COM
    SRB_AGENT_OUTPUTS;
    STAMP_END(15);
    STAMP_FLUSH(agent);
    if (tid == 0) {
        obj_out[agent] = f;
        status_out[2 * agent] = qp_flag; status_out[2 * agent + 1] = nlp_flag;
        iters_out[2 * agent] = qp_it; iters_out[2 * agent + 1] = nlp_it;
#ifdef SRB_DIAG_POLISH_OUT
        obj_out[agent] = dg_eqr; iters_out[2 * agent] = dg_bits;
#endif
    }
    LCK_REPORT(2 * agent);
}


// --------------------------------------------------------------------------- polish kernel
// Launched right after the solve kernel on the same stream, same instance geometry.  It rebuilds
// the agent's basis and term rows (SRB_AGENT_SETUP), takes the NLP result from x_out and the
// interior-point active set / multipliers from zpol_g, and replaces x, obj, alpha and the NLP
// status (-> OPTIMAL) only when the polish is accepted.  A kernel of its own: inside the solve
// kernel the polish's registers competed with the interior-point loop's and pushed its spills
// from 8 to 100-200 (configs[2] 0.40 -> 0.47-0.66 ms); here the loop is untouched.
template <int NZL, int TS, int NW, int NC, int CC, int KC, int MV = 0>
__device__ __forceinline__ void polish_agent(const SrbKParams &prm, int agent,
                const double *__restrict__ x0g, const double *__restrict__ refg, const double *__restrict__ footg,
                const double *__restrict__ obstacles, const double *__restrict__ nbr_state,
                double *__restrict__ x_out, double *__restrict__ obj_out, int *__restrict__ status_out,
                const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,
                const int *__restrict__ sel_g, const float *__restrict__ zpol_g, int zstride,
                const double *__restrict__ nbr_plan, double *__restrict__ plan_out,
                const double *__restrict__ obs_vel, const double *__restrict__ obs_eps,
                const double *__restrict__ agent_rad, const double *__restrict__ agent_pad, int agent_offset,
                double *lds)
{
    SRB_AGENT_LAYOUT;
#ifdef SRB_STAMPS
    unsigned long long *stamp_lds = nullptr;                // (the stamps build times the solve kernel only)
#endif
    double *Rt = R + rC * LDR;
    using TK = SlotTrips<NTH, TS, NC, CC, KC>;
    (void)xb; (void)dxv; (void)th; (void)tol; (void)wv;
    const int st1 = status_out[2 * agent + 1];
    if (!prm.use_nlp || st1 == 1 || st1 == 3) return;          // the whole workgroup: no usable iterate to polish
    // the solve's outputs first (x into xsv, which the setup does not clear; the exported active set
    // / multipliers into registers), so their HBM latency overlaps the setup
    const float *zp = zpol_g + (size_t)agent * zstride;
    float zv[TS][2];
#pragma unroll
    for (int t = 0; t < TS; t++) {
        const int sl = tid + NTH * t;
#pragma unroll
        for (int r = 0; r < 2; r++) zv[t][r] = (sl < S) ? zp[2 * sl + r] : 0.0f;
    }
    for (int v = tid; v < n; v += NTH) xsv[v] = x_out[(size_t)agent * n + v];
    SRB_AGENT_SETUP;
    SYNC();
    for (int v = tid; v < n; v += NTH) xs[v] = xsv[v];
    SYNC();
    POLDBG_IN(zp, S, xs, n);
    double Mi[NZL], dxi[NZL];
    // ---------------- active-set polish of the NLP result (oracle/nlp_ipm.c `polish`, the same rules) ----------------
    // Near its round-off floor the barrier system's active rows carry z/s ~ 1e14, so the
    // interior-point iterate stops up to ~1e-4 from the optimum along soft directions.  Rows
    // with s * KAPPA < z are taken as the active set A and min f s.t. Aeq x = beq, g_A(x) = h_A
    // is solved by Newton steps on its KKT system regularised by 1 / RHO:
    //   Z'(H_L + RHO J_A'J_A)Z dxi = -Z'(grad f + J_A'(z_A + RHO c_A)),  z_A += RHO (c_A + J_A Z dxi)
    // -- the interior-point machinery with weight RHO on the active rows, 0 on the others --
    // whose fixed point is the exact KKT point of that active set; at most SRB_POLISH_IT steps,
    // fewer once a correction is below SRB_POLISH_DXTOL.  Accepted (OPTIMAL) only when primal
    // feasible, dual feasible and converged; otherwise the most negative multiplier leaves A,
    // violated rows join, and the next pass starts again from the interior-point result (at
    // most SRB_POLISH_PASSES); a rejected polish leaves that result.  The slots are rebuilt
    // here (the interior-point slot state is dead); their fields ds = active mask, dz = z_A,
    // r3 = row value g - h, jd = g(x), s = the inactive rows' interior-point weight z/s, kept in
    // the Hessian only (a proximal term: the fixed point is unchanged, and the reduced matrix
    // stays definite along directions no active row pins, lambda with four contacts).
    {
        const int nts = (S + NTH - 1) / NTH;
        const int cnt = rU, nko = NKP;
        Slot P[TS];
#pragma unroll
        for (int t = 0; t < TS; t++) {
            Slot &q = P[t];
            const int sl = tid + NTH * t;
            slot_init(q, sl, prm, TL, ref, sE, sV, sO, S, rC, rO, K, TT);
            SRB_SLOT_LCK(q, sl);
            slot_stage<TK>(q, t, n, true, TT);
            if (SK_ISP(q, t, K_OBS)) { const int o = sl - sO; q.a0 = obs[2 * o]; q.a1 = obs[2 * o + 1]; q.h[0] = -eps[o % K]; }
#pragma unroll
            for (int r = 0; r < 2; r++)
            if (SK_TWO(t) || r == 0) {
                const double v = (t < nts && sl < S) ? (double)zv[t][r] : 0.0;
                q.ds[r] = (v > 0.0) ? 1.0 : 0.0;
                q.dz[r] = fmax(v, 0.0);
                q.s[r] = fmax(-v, 0.0);
            }
        }
        bool accepted = false;
#ifdef SRB_DIAG_POLISH_OUT
        double dg_eqr = -1.0;
        int dg_bits = 0;
#endif
        SRB_POLISH_PASSES_LOOP(P);
        SYNC();
        if (accepted) {
            SRB_AGENT_OUTPUTS;
            if (tid == 0) { obj_out[agent] = f; status_out[2 * agent + 1] = 0; }
        }
    }
    LCK_REPORT(2 * agent);

}

// Kernel entries.  The solve kernel of an instance: INFIX empty and KF = 0, or INFIX f32_ and KF = 1 for the
// fp32-factor instances (SRB_OPT_KKT_FP32_MU > 0 selects them): configs[4]'s "fp32 KKT with fp64 iterative-refine
// residuals" -- the reduced Newton matrix assembled and refined against in fp64, inverted in fp32 while the
// complementarity mu is above prm.kkt32_mu, in fp64 below
#define SRB_NMPC_ENTRY(INFIX, KF, NZL, TS, NW, NC, CC, KC)                                                     \
    extern "C" __global__ void __launch_bounds__(64 * NW) SRB_WPE                                              \
    srb_nmpc_kernel_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                                          \
        SrbKParams prm, int n_agents, const double *__restrict__ x0g, const double *__restrict__ refg,          \
        const double *__restrict__ footg, const double *__restrict__ obstacles, int n_obs,                       \
        const double *__restrict__ nbr_state, int n_all, int agent_offset, double *__restrict__ x_qp_out,        \
        double *__restrict__ x_out, double *__restrict__ obj_out, int *__restrict__ status_out,                 \
        int *__restrict__ iters_out, const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,       \
        const int *__restrict__ sel_g, float *__restrict__ zpol_g, int zstride,                               \
        const double *__restrict__ nbr_plan, double *__restrict__ plan_out)                                    \
    {                                                                                                          \
        extern __shared__ __attribute__((aligned(16))) double lds[];                                           \
        const int agent = xcd_agent(blockIdx.x, gridDim.x);                                                   \
        if (agent >= n_agents) return;                                                                         \
        nmpc_agent<NZL, TS, NW, NC, CC, KC, KF>(prm, agent, x0g, refg, footg, obstacles, n_obs, nbr_state, n_all, agent_offset, \
                                x_qp_out, x_out, obj_out, status_out, iters_out, alpha_buf, alpha_out, sel_g, \
                                zpol_g, zstride, nbr_plan, plan_out, nullptr, nullptr, nullptr, nullptr, lds);          \
    }
#define SRB_POLISH_ENTRY(NZL, TS, NW, NC, CC, KC)                                                              \
    extern "C" __global__ void __launch_bounds__(64 * NW) SRB_WPE                                              \
    srb_polish_kernel_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                                               \
        SrbKParams prm, int n_agents, const double *__restrict__ x0g, const double *__restrict__ refg,          \
        const double *__restrict__ footg, const double *__restrict__ obstacles,                                 \
        const double *__restrict__ nbr_state, double *__restrict__ x_out, double *__restrict__ obj_out,          \
        int *__restrict__ status_out, const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,     \
        const int *__restrict__ sel_g, const float *__restrict__ zpol_g, int zstride,                         \
        const double *__restrict__ nbr_plan, double *__restrict__ plan_out)                                    \
    {                                                                                                          \
        extern __shared__ __attribute__((aligned(16))) double lds[];                                           \
        const int agent = xcd_agent(blockIdx.x, gridDim.x);                                                   \
        if (agent >= n_agents) return;                                                                         \
        polish_agent<NZL, TS, NW, NC, CC, KC>(prm, agent, x0g, refg, footg, obstacles, nbr_state, x_out, obj_out,          \
                                  status_out, alpha_buf, alpha_out, sel_g, zpol_g, zstride, nbr_plan, plan_out, nullptr, nullptr, nullptr, nullptr, 0, lds); \
    }
// The table instances (srb_moving.obs_vel, srb_sizes.obs_eps, srb_agent_sizes.agent_rad / agent_pad; MV = 1): the
// same kernels with the four tables as further arguments (each may be null; the polish kernel, which has no
// agent_offset of its own, takes that too: the agent's own row) and the arms of SRB_AGENT_OBSTACLES that read them
// compiled in, named srb_nmpc_kernel_mv_* / srb_polish_kernel_mv_*.
// Instances of their own, as the fp32-factor instances are, and in code objects of their own (SRB_PART 4 .. 7): with
// the argument on the default instances the default bench step measured 0.5 % and config 5 0.3 % slower than the
// parent, outside its run-to-run spread, so the default instances keep their code.
#define SRB_NMPC_ENTRY_MV(INFIX, KF, NZL, TS, NW, NC, CC, KC)                                                  \
    extern "C" __global__ void __launch_bounds__(64 * NW) SRB_WPE                                              \
    srb_nmpc_kernel_mv_##INFIX##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                                       \
        SrbKParams prm, int n_agents, const double *__restrict__ x0g, const double *__restrict__ refg,          \
        const double *__restrict__ footg, const double *__restrict__ obstacles, int n_obs,                       \
        const double *__restrict__ nbr_state, int n_all, int agent_offset, double *__restrict__ x_qp_out,        \
        double *__restrict__ x_out, double *__restrict__ obj_out, int *__restrict__ status_out,                 \
        int *__restrict__ iters_out, const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,       \
        const int *__restrict__ sel_g, float *__restrict__ zpol_g, int zstride,                               \
        const double *__restrict__ nbr_plan, double *__restrict__ plan_out,                                    \
        const double *__restrict__ obs_vel, const double *__restrict__ obs_eps,                                \
        const double *__restrict__ agent_rad, const double *__restrict__ agent_pad)                            \
    {                                                                                                          \
        extern __shared__ __attribute__((aligned(16))) double lds[];                                           \
        const int agent = xcd_agent(blockIdx.x, gridDim.x);                                                   \
        if (agent >= n_agents) return;                                                                         \
        nmpc_agent<NZL, TS, NW, NC, CC, KC, KF, 1>(prm, agent, x0g, refg, footg, obstacles, n_obs, nbr_state, n_all, agent_offset, \
                                x_qp_out, x_out, obj_out, status_out, iters_out, alpha_buf, alpha_out, sel_g, \
                                zpol_g, zstride, nbr_plan, plan_out, obs_vel, obs_eps, agent_rad, agent_pad, lds);      \
    }
#define SRB_POLISH_ENTRY_MV(NZL, TS, NW, NC, CC, KC)                                                           \
    extern "C" __global__ void __launch_bounds__(64 * NW) SRB_WPE                                              \
    srb_polish_kernel_mv_##NZL##_##TS##_##NW##_##NC##_##CC##_##KC(                                            \
        SrbKParams prm, int n_agents, const double *__restrict__ x0g, const double *__restrict__ refg,          \
        const double *__restrict__ footg, const double *__restrict__ obstacles,                                 \
        const double *__restrict__ nbr_state, double *__restrict__ x_out, double *__restrict__ obj_out,          \
        int *__restrict__ status_out, const double *__restrict__ alpha_buf, double *__restrict__ alpha_out,     \
        const int *__restrict__ sel_g, const float *__restrict__ zpol_g, int zstride,                         \
        const double *__restrict__ nbr_plan, double *__restrict__ plan_out,                                    \
        const double *__restrict__ obs_vel, const double *__restrict__ obs_eps,                                \
        const double *__restrict__ agent_rad, const double *__restrict__ agent_pad, int agent_offset)          \
    {                                                                                                          \
        extern __shared__ __attribute__((aligned(16))) double lds[];                                           \
        const int agent = xcd_agent(blockIdx.x, gridDim.x);                                                   \
        if (agent >= n_agents) return;                                                                         \
        polish_agent<NZL, TS, NW, NC, CC, KC, 1>(prm, agent, x0g, refg, footg, obstacles, nbr_state, x_out, obj_out,       \
                                  status_out, alpha_buf, alpha_out, sel_g, zpol_g, zstride, nbr_plan, plan_out, obs_vel, obs_eps, agent_rad, agent_pad, agent_offset, lds); \
    }
#define SRB_NMPC_KERNEL(...) SRB_NMPC_ENTRY(, 0, __VA_ARGS__) SRB_POLISH_ENTRY(__VA_ARGS__)
#define SRB_NMPC_KERNEL_F32(...) SRB_NMPC_ENTRY(f32_, 1, __VA_ARGS__)
#define SRB_NMPC_KERNEL_MV(...) SRB_NMPC_ENTRY_MV(, 0, __VA_ARGS__) SRB_POLISH_ENTRY_MV(__VA_ARGS__)
#define SRB_NMPC_KERNEL_MV_F32(...) SRB_NMPC_ENTRY_MV(f32_, 1, __VA_ARGS__)

#if defined(SRB_PART) && !defined(SRB_DEV_INSTANCES)
#if SRB_PART == 0
SRB_KI_PART0(SRB_NMPC_KERNEL)
#elif SRB_PART == 1
SRB_KI_PART1(SRB_NMPC_KERNEL)
#elif SRB_PART == 2
SRB_KI_PART2(SRB_NMPC_KERNEL)
SRB_KF32_PART2(SRB_NMPC_KERNEL_F32)
#elif SRB_PART == 3
SRB_KI_PART3(SRB_NMPC_KERNEL)
SRB_KF32_PART3(SRB_NMPC_KERNEL_F32)
#elif SRB_PART == 4     // parts 4 .. 7: the moving-obstacle instances of parts 0 .. 3
SRB_KI_PART0(SRB_NMPC_KERNEL_MV)
#elif SRB_PART == 5
SRB_KI_PART1(SRB_NMPC_KERNEL_MV)
#elif SRB_PART == 6
SRB_KI_PART2(SRB_NMPC_KERNEL_MV)
SRB_KF32_PART2(SRB_NMPC_KERNEL_MV_F32)
#else
SRB_KI_PART3(SRB_NMPC_KERNEL_MV)
SRB_KF32_PART3(SRB_NMPC_KERNEL_MV_F32)
#endif
#else
SRB_KERNEL_INSTANCES(SRB_NMPC_KERNEL)
#ifndef SRB_DEV_INSTANCES
SRB_KF32_INSTANCES(SRB_NMPC_KERNEL_F32)
SRB_KERNEL_INSTANCES(SRB_NMPC_KERNEL_MV)
SRB_KF32_INSTANCES(SRB_NMPC_KERNEL_MV_F32)
#endif
#endif

// The selection kernels (srb_select.hip) are compiled into the code object of part 0 (or of the single-unit
// builds), not one of their own: as a separate object, with every kernel's machine code unchanged, the default
// bench step measured 0.3-0.6 % slower in three of three A/B runs against the library before the move (the
// selection kernel runs right before the solve kernel of part 0 every step), and not with this layout.
#if !defined(SRB_PART) || SRB_PART == 0
#include "srb_select.hip"
#endif
