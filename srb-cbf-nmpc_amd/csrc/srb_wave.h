// Wavefront helpers shared by the gfx950 kernels of this library (NMPC solve, selection, SRB-12,
// low-level CLF-QP): the XCD-aware agent mapping, DPP/permlane reductions and argmins, readlane and
// row_newbcast broadcasts, a refined reciprocal.  Header-only, device code.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

#ifndef WAVE
#define WAVE 64
#endif
#ifndef SRB_USE_DPP     // DPP row_newbcast broadcasts in the reduced solve (0: readlane / LDS forms)
#define SRB_USE_DPP 1
#endif
// The row broadcast folded into the FMA (one v_fmac_f64_dpp row_newbcast instead of v_mov_b64_dpp + v_fma_f64) in the
// DPP Gauss-Jordan (srb_gj.h) and the DPP reduced solve (srb_solve.h); 0 keeps the bc16() + fma() text everywhere.
// Only under SRB_USE_DPP and NZL <= 16; which instances take it: srb_dpp_fold below (2, a diagnostic build: the
// run-time NZL <= 16 instances too -- the comparison of profiles/dpp_fold_static.txt).
#ifndef SRB_DPP_FOLD
#define SRB_DPP_FOLD 1
#endif

typedef double d4 __attribute__((ext_vector_type(4)));

// f(integral_constant<int, I>) for I = 0 .. n - 1 in turn
template <class F, int... I>
__device__ __forceinline__ void srb_static_for(std::integer_sequence<int, I...>, F &&f)
{
    (f(std::integral_constant<int, I>{}), ...);
}

// Whether the reduced matrix of bound NZL with NZE steps compiled in takes the folded forms: the one-block shapes whose
// reduced size is compiled in (NZE < NZL: 12_4_1_10_2_11, 12_1_4_10_2_3 and their f32, table and polish kernels).  The
// run-time instances (NZE = NZL) keep the bc16() + fma() text (profiles/dpp_fold_static.txt).
constexpr bool srb_dpp_fold(int NZL, int NZE)
{
    return SRB_DPP_FOLD && SRB_USE_DPP && NZL <= 16 && (NZE == 8 || NZE == 11 || NZE == 12 || NZE == 16) &&
           (NZE < NZL || SRB_DPP_FOLD == 2);
}

// Agent of workgroup b in a grid of n one-agent workgroups, XCD-aware: the dispatcher deals
// workgroups round-robin over the 8 XCDs (MI355X_MICROARCH.md, "Workgroup dispatch"; observed, not
// promised -- only the traffic depends on it), so b and b + 8 share an L2.  Workgroups b = 8 j + x take
// the x-th contiguous block of agents: neighbouring agents' inputs share 128-B lines, which a
// round-robin assignment fetched once into each of up to four L2s (configs[2]: x0, ref, foot and the
// selection rows 1.09 -> 0.73 MB per launch, tools/ubench/kernarg_fetch.hip).
// A bijection of [0, n) for every n.
__device__ __forceinline__ int xcd_agent(int b, int n)
{
    const int q = n >> 3, r = n & 7, x = b & 7;
    return x * q + min(x, r) + (b >> 3);
}

// Barrier of the NW-wave workgroup.  NW = 1 (one agent per wave, the large-batch instances): the LDS
// accesses of one wavefront execute in issue order, so a wavefront-scope fence (no s_waitcnt) and a wave
// barrier suffice -- __syncthreads would wait for every outstanding LDS store first.  (Every SYNC site
// sits in a function templated on NW.)
// What this relies on: (1) LLVM IR -- a fence, whatever its scope, orders the thread's memory
// operations: no load or store is moved across it (an acq_rel fence is a read-write of all memory for
// alias analysis), so the ISA keeps the source order of the LDS accesses around SYNC; the wave barrier
// is IntrNoMem (a convergence point only) and is not what orders them.  (2) The AMDGPU memory model
// (LLVM AMDGPUUsage, memory model for GFX942 / GFX950): the LDS operations of one wavefront are performed
// in issue order, so a ds_read by any lane observes an earlier ds_write of the same wave without an
// s_waitcnt; the compiler still waits (lgkmcnt) before a loaded value is used.
template <int NW>
__device__ __forceinline__ void srb_sync()
{
    if constexpr (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// --------------------------------------------------------------------------- wave helpers
// Cross-lane traffic stays in the VALU: DPP row permutations for the 16-lane rows and
// gfx950's v_permlane16/32_swap across rows.  Every lane ends with the bit-identical
// result (each stage combines a pair with a commutative op), so branches on it are uniform.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// the two halves of a permlane swap of v with itself: {v, partner} in some order
template <int W>
__device__ __forceinline__ void swap_d(double v, double &a, double &b)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    auto l = (W == 16) ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false) : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h = (W == 16) ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false) : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    a = __longlong_as_double((long long)(((unsigned long long)h[0] << 32) | l[0]));
    b = __longlong_as_double((long long)(((unsigned long long)h[1] << 32) | l[1]));
}
#define SRB_WAVE_REDUCE(NAME, OP)                                                  \
    __device__ __forceinline__ double NAME(double v)                               \
    {                                                                              \
        v = OP(v, dpp_d<0xB1>(v));   /* quad_perm [1,0,3,2] */                     \
        v = OP(v, dpp_d<0x4E>(v));   /* quad_perm [2,3,0,1] */                     \
        v = OP(v, dpp_d<0x141>(v));  /* row_half_mirror     */                     \
        v = OP(v, dpp_d<0x140>(v));  /* row_mirror          */                     \
        double a, b;                                                               \
        swap_d<16>(v, a, b); v = OP(a, b);                                         \
        swap_d<32>(v, a, b); return OP(a, b);                                      \
    }
__device__ __forceinline__ double op_add(double a, double b) { return a + b; }
SRB_WAVE_REDUCE(wsum, op_add)
SRB_WAVE_REDUCE(wmin, fmin)
SRB_WAVE_REDUCE(wmax, fmax)
// NV independent wave reductions interleaved stage by stage (one DPP/permlane latency per
// stage for all of them); bit i of MX selects max (1) or sum (0) for v[i].
template <int NV, unsigned MX>
__device__ __forceinline__ void wred(double (&v)[NV])
{
#define SRB_RED_STAGE(GET)                                                                      \
    _Pragma("unroll") for (int i = 0; i < NV; i++) {                                            \
        const double t_ = GET;                                                                  \
        v[i] = ((MX >> i) & 1u) ? fmax(v[i], t_) : v[i] + t_;                                   \
    }
    SRB_RED_STAGE(dpp_d<0xB1>(v[i]))
    SRB_RED_STAGE(dpp_d<0x4E>(v[i]))
    SRB_RED_STAGE(dpp_d<0x141>(v[i]))
    SRB_RED_STAGE(dpp_d<0x140>(v[i]))
#undef SRB_RED_STAGE
#pragma unroll
    for (int i = 0; i < NV; i++) {
        double a, b;
        swap_d<16>(v[i], a, b);
        v[i] = ((MX >> i) & 1u) ? fmax(a, b) : a + b;
    }
#pragma unroll
    for (int i = 0; i < NV; i++) {
        double a, b;
        swap_d<32>(v[i], a, b);
        v[i] = ((MX >> i) & 1u) ? fmax(a, b) : a + b;
    }
}
// wred over all NW waves of the workgroup: per-wave DPP reduction, then lane 0 of every wave
// publishes to `scr` (NW x NV doubles, one scratch block per call site) and every thread
// combines the NW partials in the same order (identical results on every lane and wave).
template <int NV, unsigned MX, int NW>
__device__ __forceinline__ void wred_x(double (&v)[NV], double *scr, int tid)
{
    wred<NV, MX>(v);
    if constexpr (NW > 1) {
        if ((tid & 63) == 0)
#pragma unroll
            for (int i = 0; i < NV; i++) scr[(tid >> 6) * NV + i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; i++) {
            double r = scr[i];
#pragma unroll
            for (int w = 1; w < NW; w++) r = ((MX >> i) & 1u) ? fmax(r, scr[w * NV + i]) : r + scr[w * NV + i];
            v[i] = r;
        }
    }
}
// sum over the lanes that share (lane mod W), W = 16 or 32: permlane butterflies only
__device__ __forceinline__ double chunk_sum16(double v)
{
    double a, b;
    swap_d<32>(v, a, b); v = a + b;
    swap_d<16>(v, a, b); return a + b;
}
__device__ __forceinline__ double chunk_sum32(double v)
{
    double a, b;
    swap_d<32>(v, a, b); return a + b;
}
// value of lane `lane` (wave-uniform index) -> wave-uniform value
__device__ __forceinline__ double readlane_d(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// 1/x from the hardware estimate (v_rcp_f64) refined by two Newton steps: within an ulp
// or two of the IEEE quotient, a handful of FMAs instead of the division sequence.
__device__ __forceinline__ double rcp_d(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    return r;
}
__device__ __forceinline__ int rnd4(int x) { return (x + 3) & ~3; }

// value of lane k of this lane's 16-lane row: one v_mov_b64_dpp row_newbcast:k (gfx90a+),
// a VALU result the next instruction can consume -- no SGPR round trip as with readlane.
// k must fold to a constant (unrolled loops).
// (row_newbcast writes every lane, so the "old" operand is never used: passing v with bound_ctrl
// lets the compiler emit the DPP move alone, without first zeroing its destination)
__device__ __forceinline__ double bc16(double v, int k)
{
    switch (k) {
#define SRB_BC(K) case K: return __builtin_amdgcn_update_dpp(v, v, 0x150 + K, 0xf, 0xf, true);
    SRB_BC(0) SRB_BC(1) SRB_BC(2) SRB_BC(3) SRB_BC(4) SRB_BC(5) SRB_BC(6) SRB_BC(7)
    SRB_BC(8) SRB_BC(9) SRB_BC(10) SRB_BC(11) SRB_BC(12) SRB_BC(13) SRB_BC(14) default: SRB_BC(15)
#undef SRB_BC
    }
}

// --------------------------------------------------------------------------- argmin
// (d, index) lexicographic wave argmin; every lane gets the winner
__device__ __forceinline__ void lexmin(double &d, int &idx, double od, int oi)
{
    if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
}
__device__ __forceinline__ void wargmin(double &d, int &idx)
{
    // the wsum pattern (DPP within 16-lane rows, permlane swaps across them) on the pair
#define SRB_ARG_DPP(CTRL) lexmin(d, idx, dpp_d<CTRL>(d), __builtin_amdgcn_update_dpp(0, idx, CTRL, 0xf, 0xf, false))
    SRB_ARG_DPP(0xB1); SRB_ARG_DPP(0x4E); SRB_ARG_DPP(0x141); SRB_ARG_DPP(0x140);
#undef SRB_ARG_DPP
    double a, b;
    swap_d<16>(d, a, b);
    auto i16 = __builtin_amdgcn_permlane16_swap((unsigned)idx, (unsigned)idx, false, false);
    d = a; idx = (int)i16[0]; lexmin(d, idx, b, (int)i16[1]);
    swap_d<32>(d, a, b);
    auto i32 = __builtin_amdgcn_permlane32_swap((unsigned)idx, (unsigned)idx, false, false);
    d = a; idx = (int)i32[0]; lexmin(d, idx, b, (int)i32[1]);
}

// The same (d, index) lexicographic wave argmin as wargmin, by a double minimum and a ballot (round 6,
// tools/ubench/knn_phase.hip): one fmin per stage instead of the pair's three compares and three selects;
// the index comes from the one lane holding the minimum (v_readlane), or -- when several lanes hold it: an
// exact distance tie, or every head exhausted (+inf) -- from an integer minimum over those lanes' indices.
// Every lane ends with the same (d, idx).  d is never NaN here (knn_select_k offers no NaN keys).
__device__ __forceinline__ int wmin_i(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false));
    auto p16 = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    v = min((int)p16[0], (int)p16[1]);
    auto p32 = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return min((int)p32[0], (int)p32[1]);
}
__device__ __forceinline__ void wargmin_b(double &d, int &idx)
{
    const double m = wmin(d);
    const unsigned long long tie = __ballot(d == m);
    int w;
    if (__popcll(tie) == 1) w = __builtin_amdgcn_readlane(idx, __ffsll((long long)tie) - 1);
    else w = wmin_i((d == m) ? idx : 0x7fffffff);
    d = m; idx = w;
}

// wargmin over the NW waves of the workgroup: per-wave DPP argmin, lane 0 of every wave
// publishes (d, idx) to scr[2 NW], every thread combines the partials in wave order
template <int NW>
__device__ __forceinline__ void wargmin_x(double &d, int &idx, double *scr, int tid)
{
    wargmin(d, idx);
    if constexpr (NW > 1) {
        if ((tid & 63) == 0) { scr[2 * (tid >> 6)] = d; scr[2 * (tid >> 6) + 1] = (double)idx; }
        __syncthreads();
        d = scr[0]; idx = (int)scr[1];
#pragma unroll
        for (int w = 1; w < NW; w++) lexmin(d, idx, scr[2 * w], (int)scr[2 * w + 1]);
    }
}
