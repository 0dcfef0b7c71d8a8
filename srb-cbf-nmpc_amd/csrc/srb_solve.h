// Reduced Newton solve of the NMPC solve kernel (srb_kernels.hip): the load of the reduced matrix one row per lane
// (gj_load, mrow), the solve with its explicit inverse and iterative refinement (la_solve), and the dot products of
// LDS term rows with the solution (row_load, row_sum, row_dot).  Header-only device code, so that
// tools/ubench/gj_bench.hip times this text and not a copy of it.
#pragma once
#include "srb_kernel_params.h"
#include "srb_wave.h"
#include "srb_gj.h"

// dot of LDS term row (lane-parallel rows) with a wave-uniform vector held in registers: the whole row
// first (row_load: its loads in flight together, one LDS round trip a row -- written element by element into
// the FMAs, the compiler ran every pair of elements through one shared temporary, a round trip a pair), then
// the sums in their fixed order (row_sum)
template <int NZE>
__device__ __forceinline__ void row_load(const double *row, double (&a)[NZE])
{
#pragma unroll
    for (int j = 0; j < NZE; j++) a[j] = row[j];
}
template <int NZL, int NZE = NZL>
__device__ __forceinline__ double row_sum(const double (&a)[NZE], const double (&v)[NZL])
{
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j + 1 < NZE; j += 2) { s0 = fma(a[j], v[j], s0); s1 = fma(a[j + 1], v[j + 1], s1); }
    if (NZE & 1) s0 = fma(a[NZE - 1], v[NZE - 1], s0);
    return s0 + s1;
}
template <int NZL, int NZE = NZL>
__device__ __forceinline__ double row_dot(const double *row, const double (&v)[NZL])
{
    double a[NZE];
    row_load<NZE>(row, a);
    __builtin_amdgcn_sched_barrier(0);
    return row_sum<NZL, NZE>(a, v);
}

// row of the reduced matrix a lane holds: lane (NZL > 16, readlane Gauss-Jordan) or lane & 15
// (NZL <= 16: every 16-lane row of the wave holds the whole matrix, DPP broadcasts)
template <int NZL>
__device__ __forceinline__ int mrow(int lane) { return (NZL <= 16 && SRB_USE_DPP) ? (lane & 15) : lane; }

// lane i (< NZL) loads row i of H (+ delta * Z'Z) with identity padding
template <int NZL, int NZE = NZL>
__device__ __forceinline__ void gj_load(double (&A)[NZL], const double *H, const double *ZtZ, double delta, int nz, int lane)
{
    constexpr int LDH = NZL + 1;
    lane = mrow<NZL>(lane);
    const int i = (lane < NZL) ? lane : 0;
#pragma unroll
    for (int j = 0; j < NZL; j++) {
        if (j >= NZE) { A[j] = (lane == j) ? 1.0 : 0.0; continue; }
        double v = H[i * LDH + j];
        if (delta != 0.0) v = fma(delta, ZtZ[i * LDH + j], v);
        A[j] = (lane < nz && j < nz) ? v : ((lane == j) ? 1.0 : 0.0);
    }
}

// acc += sum_j bcast_j(x) m[j] (NEG: -m[j]), j = 0 .. NZE - 1 in turn, bcast_j: lane j of this lane's 16-lane row -- a
// matvec of the DPP la_solve below with the broadcast folded into the FMA (SRB_DPP_FOLD): one statement of NZE
// v_fmac_f64_dpp acc, x, m[j] row_newbcast:j, the same fused operations in the same order as acc = fma(m[j], bc16(x, j), acc).
// Wait states as srb_gj.h gj_fold_step: only x is DPP-read; it may just have been written by compiler code (a
// v_cndmask: rr of the lanes >= nz; an LDS load's select; an AGPR un-spill), so the statement opens with s_nop 1; and acc
// is DPP-read next (by the following matvec, or by the compiler's bc16 of the result), so it closes with s_nop 1.
// All 64 lanes must be active (row_newbcast reads another lane): every call site of la_solve is wave-uniform.
#define SRB_MV(J, S) "v_fmac_f64_dpp %[acc], %[x], " S "%[m" #J "] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define SRB_MI(J) [m##J] "v"(m[J])
#define SRB_MV8(S) SRB_MV(0, S) SRB_MV(1, S) SRB_MV(2, S) SRB_MV(3, S) SRB_MV(4, S) SRB_MV(5, S) SRB_MV(6, S) SRB_MV(7, S)
#define SRB_MV11(S) SRB_MV8(S) SRB_MV(8, S) SRB_MV(9, S) SRB_MV(10, S)
#define SRB_MV12(S) SRB_MV11(S) SRB_MV(11, S)
#define SRB_MV16(S) SRB_MV12(S) SRB_MV(12, S) SRB_MV(13, S) SRB_MV(14, S) SRB_MV(15, S)
#define SRB_MI8 SRB_MI(0), SRB_MI(1), SRB_MI(2), SRB_MI(3), SRB_MI(4), SRB_MI(5), SRB_MI(6), SRB_MI(7)
#define SRB_MI11 SRB_MI8, SRB_MI(8), SRB_MI(9), SRB_MI(10)
#define SRB_MI12 SRB_MI11, SRB_MI(11)
#define SRB_MI16 SRB_MI12, SRB_MI(12), SRB_MI(13), SRB_MI(14), SRB_MI(15)
#define SRB_MST(N, S) asm volatile("s_nop 1\n\t" SRB_MV##N(S) "s_nop 1" : [acc] "+v"(acc) : [x] "v"(x), SRB_MI##N)
#define SRB_MSTN(N) do { if constexpr (NEG) SRB_MST(N, "-"); else SRB_MST(N, ""); } while (0)
template <int NZE, bool NEG, int NM>
__device__ __forceinline__ void mv_fold(double &acc, double x, const double (&m)[NM])
{
    static_assert(NZE <= NM && (NZE == 8 || NZE == 11 || NZE == 12 || NZE == 16), "mv_fold: the reduced sizes of the shipped instances");
    if constexpr (NZE == 8) SRB_MSTN(8);
    else if constexpr (NZE == 11) SRB_MSTN(11);
    else if constexpr (NZE == 12) SRB_MSTN(12);
    else SRB_MSTN(16);
}
#undef SRB_MV
#undef SRB_MI
#undef SRB_MV8
#undef SRB_MV11
#undef SRB_MV12
#undef SRB_MV16
#undef SRB_MI8
#undef SRB_MI11
#undef SRB_MI12
#undef SRB_MI16
#undef SRB_MST
#undef SRB_MSTN

// Newton solve in the reduced space: out = (Hs + dl Zs)^-1 g with one step of iterative refinement
// (y = M g; y += M (g - Hs y)): the explicit inverse alone is not backward stable, and near
// the end of an interior-point solve Hs carries barrier weights of 1e8..1e12.
// g, y, r, out: LDS vectors (zero beyond nz).  Returns out in registers (uniform).
// KF (the fp32-factor instances, configs[4] "fp32 KKT with fp64 iterative-refine residuals"): `nref` steps of
// refinement instead of SRB_REFINE, run-time (more while M is the fp32 inverse); the product instances (KF = 0)
// keep the compile-time count and are unchanged.
// FOLD (srb_dpp_fold, srb_wave.h): the three matvecs of the DPP branch as mv_fold statements; delta != 0, the KF
// refinement loop and polish_stationary's call take the same code.
template <int NZL, int NW, int NZE = NZL, int KF = 0, bool FOLD = srb_dpp_fold(NZL, NZE)>
__device__ __forceinline__ void la_solve(const double (&M)[NZL], const double *Hs, const double *Zs, double dl, const double *g,
                                         double *y, double *r, double *out, double (&res)[NZL], int nz, int lane, int nref = SRB_REFINE)
{
    constexpr int LDH = NZL + 1;
    if constexpr (NZL <= 16 && SRB_USE_DPP) {
        // rows replicated per 16-lane row: the three vector broadcasts are DPP moves, no LDS
        // round trip or barrier
        const int i = lane & 15;
        const double gi = (i < nz) ? g[i] : 0.0;         // g is zero beyond nz
        // this lane's row of the matrix the refinement multiplies by (independent of y): loaded once, ahead of
        // the first product, instead of one element per FMA of the residual
        double hr[NZE];
#pragma unroll
        for (int j = 0; j < NZE; j++) hr[j] = Hs[i * LDH + j];
        if (dl != 0.0) {                     // the NLP's inertia shift, applied on the fly (H stays unshifted)
#pragma unroll
            for (int j = 0; j < NZE; j++) hr[j] = fma(dl, Zs[i * LDH + j], hr[j]);
        }
        double y0 = 0.0;
#pragma unroll
        for (int j = 0; j < NZE; j++)
            if constexpr (!FOLD) y0 = fma(M[j], bc16(gi, j), y0);
        if constexpr (FOLD) mv_fold<NZE, false>(y0, gi, M);
        // SRB_REFINE steps of iterative refinement with fp64 residuals (the KF instances: nref)
        double y1 = y0;
        const int nr = KF ? nref : SRB_REFINE;
#pragma unroll
        for (int it = 0; it < (KF ? 8 : SRB_REFINE); it++) {
            if (KF && it >= nr) break;
            double rr = gi;
#pragma unroll
            for (int j = 0; j < NZE; j++)
                if constexpr (!FOLD) rr = fma(-hr[j], bc16(y1, j), rr);
            if constexpr (FOLD) mv_fold<NZE, true>(rr, y1, hr);
            if (i >= nz) rr = 0.0;
#pragma unroll
            for (int j = 0; j < NZE; j++)
                if constexpr (!FOLD) y1 = fma(M[j], bc16(rr, j), y1);
            if constexpr (FOLD) mv_fold<NZE, false>(y1, rr, M);
        }
#pragma unroll
        for (int j = 0; j < NZL; j++) res[j] = (j < NZE) ? bc16(y1, j) : 0.0;
        return;
    }
    const int i = (lane < NZL) ? lane : 0;
    double gv[NZL];
#pragma unroll
    for (int j = 0; j < NZE; j++) gv[j] = g[j];
    double y0 = 0.0;
#pragma unroll
    for (int j = 0; j < NZE; j++) y0 = fma(M[j], gv[j], y0);
    double y1 = y0;
    const int nr = KF ? nref : SRB_REFINE;
    for (int it = 0; it < nr; it++) {
        if (it > 0) srb_sync<NW>();              // every lane has read the previous r
        if (lane < nz) y[lane] = y1;
        srb_sync<NW>();
        double rr = (lane < nz) ? g[lane] : 0.0;
        if (dl != 0.0) {
#pragma unroll
            for (int j = 0; j < NZE; j++) rr = fma(-fma(dl, Zs[i * LDH + j], Hs[i * LDH + j]), y[j], rr);
        } else {
#pragma unroll
            for (int j = 0; j < NZE; j++) rr = fma(-Hs[i * LDH + j], y[j], rr);
        }
        if (lane < nz) r[lane] = rr;
        srb_sync<NW>();
#pragma unroll
        for (int j = 0; j < NZE; j++) y1 = fma(M[j], r[j], y1);
    }
    if (lane < nz) out[lane] = y1;
    srb_sync<NW>();
#pragma unroll
    for (int j = 0; j < NZL; j++) res[j] = (j < NZE) ? out[j] : 0.0;
}
