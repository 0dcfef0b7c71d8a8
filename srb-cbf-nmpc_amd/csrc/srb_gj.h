// Register Gauss-Jordan inverses of an SPD matrix held one row per lane (NMPC reduced Newton matrix, low-level
// CLF-QP Schur complement): readlane, fp32 and DPP forms.  Header-only, device code.
#pragma once
#include "srb_wave.h"

// In-place inverse of the nz x nz SPD matrix held one row per lane (lane i: A[0..NZL)),
// rows/columns >= nz padded with the identity.  Step k broadcasts the pivot row by
// v_readlane and every other lane eliminates column k from its row; the pivot row itself is
// not scaled (each lane keeps 1 / its own pivot and scales its row once at the end), so a
// step is one multiplier and one FMA per entry.  The pivots are those of LDL' in natural
// order, so pivot <= 0 <=> not positive definite; regularise != 0 applies iSWIFT's dynamic
// pivot regularisation (ldl.c:320-321: |D_kk| <= 1e-14 -> 1e-7).  Returns 0 on success.
// Rows may be replicated: with NZL <= 16 (and SRB_USE_DPP) every 16-lane row of the wave holds
// the whole matrix (lane l: matrix row l & 15) for the DPP solves that follow (la_solve); the
// broadcasts read the first copy, and each copy applies the same operations (bit-identical).
// The solve kernels call gj_factor (below), which takes the DPP row_newbcast form of this elimination
// (gj_invert_dpp) where the rows are replicated: 2638 against 3114 cycles for NZL = 12 on MI355X, 2283 against 2702
// with NZE = 11 (tools/ubench/gj_bench.hip, profiles/dpp_fold_ubench.txt; 3546 while the broadcast still zeroed its
// destination first), and with the broadcast folded into the FMA (gj_invert_dpp_fold) 2210 and 1975.  A step here is
// 22 v_readlane_b32 and 11 FMAs plus the pivot chain; the chain's dependent FMAs issue at the full 4-cycle
// rate, so interleaving them with the step's bulk gains nothing (profiles/factor_chain_ubench.txt).
__device__ __forceinline__ float readlane_f(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
// the fp32 form of gj_invert below (same steps), on the matrix rounded to fp32
template <int NZL>
__device__ __forceinline__ int gj_invert_f32(double (&Ad)[NZL], int lane, int regularise)
{
    float A[NZL];
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] = (float)Ad[j];
    int fail = 0;
    float cs = 1.0f;
#pragma unroll
    for (int k = 0; k < NZL; k++) {
        float piv = readlane_f(A[k], k);
        if (regularise && piv <= 1e-14f && piv == piv) piv = 1e-7f;
        fail |= !(piv > 0.0f);
        const float inv = 1.0f / piv;
        float rk[NZL];
#pragma unroll
        for (int j = 0; j < NZL; j++) rk[j] = (j == k) ? 0.0f : readlane_f(A[j], k);
        const bool me = lane == k;
        const float f = me ? 0.0f : A[k] * inv;
#pragma unroll
        for (int j = 0; j < NZL; j++)
            if (j != k) A[j] = fmaf(-f, rk[j], A[j]);
        A[k] = me ? 1.0f : -f;
        cs = me ? inv : cs;
    }
#pragma unroll
    for (int j = 0; j < NZL; j++) Ad[j] = (double)(A[j] * cs);
    return fail;
}

template <int NZL, int NZE = NZL>
__device__ __forceinline__ int gj_invert(double (&A)[NZL], int nz, int lane, int regularise)
{
    if constexpr (NZL <= 16 && SRB_USE_DPP) lane &= 15;
    // All NZE steps run (the identity padding makes steps >= nz exact no-ops), so the whole
    // elimination is one basic block: the scheduler overlaps step k's row updates with the
    // broadcast of row k+1, whose entries are updated first.  NZE: the instance's nz when its shape
    // is compiled in (columns >= NZE are identity padding, never touched), else NZL.
    static_assert(NZE <= NZL, "NZE");
    int fail = 0;
    double cs = 1.0;
#pragma unroll
    for (int k = 0; k < NZE; k++) {
        double piv = readlane_d(A[k], k);
        if (regularise && piv <= 1e-14 && piv == piv) piv = 1e-7;
        fail |= !(piv > 0.0);
        const double inv = rcp_d(piv);
        double rk[NZL];
#pragma unroll
        for (int j = 0; j < NZE; j++) rk[j] = (j == k) ? 0.0 : readlane_d(A[j], k);
        const bool me = lane == k;
        const double f = me ? 0.0 : A[k] * inv;
#pragma unroll
        for (int jj = 0; jj < NZE; jj++) {
            const int j = (k + 1 + jj) % NZE;           // next pivot row's entries first
            if (j != k) A[j] = fma(-f, rk[j], A[j]);
        }
        A[k] = me ? 1.0 : -f;
        cs = me ? inv : cs;
    }
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] *= cs;
    return fail;
}

// NZL <= 16: the matrix is replicated in each 16-lane row of the wave (lane l holds matrix
// row l & 15) and step k broadcasts the pivot row by DPP row_newbcast:k -- one VALU move per
// entry that the row update consumes directly, so a step's critical path is the pivot's
// broadcast, reciprocal and multiplier, not the v_readlane -> SGPR -> VALU latency.  Same
// arithmetic as the readlane form above (bit-identical results).
// NZE as in gj_invert.  The pivots are per-lane values here (the same in every lane: each 16-lane row holds the
// same matrix), so the failure test is kept as a lane mask in SGPRs and the result is wave-uniform.
template <int NZL, int NZE = NZL>
__device__ __forceinline__ int gj_invert_dpp(double (&A)[NZL], int lane, int regularise)
{
    static_assert(NZL <= 16, "row_newbcast reaches within 16 lanes");
    static_assert(NZE <= NZL, "NZE");
    const int r = lane & 15;
    unsigned long long fail = 0;
    double cs = 1.0;
#pragma unroll
    for (int k = 0; k < NZE; k++) {
        double piv = bc16(A[k], k);
        if (regularise && piv <= 1e-14 && piv == piv) piv = 1e-7;
        fail |= __ballot(!(piv > 0.0));
        const double inv = rcp_d(piv);
        const bool me = r == k;
        const double f = me ? 0.0 : A[k] * inv;
#pragma unroll
        for (int jj = 0; jj < NZE; jj++) {
            const int j = (k + 1 + jj) % NZE;           // next pivot row's entries first
            if (j != k) A[j] = fma(-f, bc16(A[j], k), A[j]);
        }
        A[k] = me ? 1.0 : -f;
        cs = me ? inv : cs;
    }
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] *= cs;
    return fail != 0;
}

// gj_invert_dpp with the row broadcast folded into the FMA (SRB_DPP_FOLD): the compiler emits bc16() + fma() as a
// v_mov_b64_dpp and a v_fma_f64 and does not fold them, so the NZE - 1 row updates of step K are one assembly statement
// of   v_fmac_f64_dpp A[j], A[j], -f row_newbcast:K   (A[j] += bcast_K(A[j]) (-f): the same fused operation on the same
// three values as fma(-f, bcast_K(A[j]), A[j]), bit-identical), in gj_invert_dpp's order (K + 1 + jj) % NZE.  The pivot
// broadcast, the regularisation, the failure ballot, the reciprocal and the pivot column stay compiler code.
// Wait states (as srb_gram.h gram_group; a missing one gives wrong values with no message): a DPP-read register needs two
// wait states after a VALU write of it, and the compiler neither sees the DPP reads inside the string nor pads for them.
// The statement opens with s_nop 1 -- A[j] may just have been written by compiler code (the loads' selects, the pivot
// column of the step before, an AGPR un-spill) -- and closes with s_nop 1 -- the compiler's next instruction may be the
// v_mov_b64_dpp of the next pivot, reading A[K + 1], which the statement wrote.  Inside the statement no instruction
// reads by DPP what another one wrote.  One statement a step, so that the compiler can neither move nor copy an operand
// between the instructions.  Operands are "v": the solve kernel parks spills in AGPRs, which a DPP instruction cannot name.
// Measured (tools/ubench/gj_bench.hip, profiles/dpp_fold_ubench.txt, five launches each): 2279 .. 2283 -> 1975 .. 1979
// cycles at (NZL, NZE) = (12, 11), 2638 .. 2642 -> 2210 .. 2214 at (12, 12), 4160 -> 3100 at (16, 16), 1460 -> 1412 at (8, 8).
// EXEC: row_newbcast reads another lane, so all 64 lanes must be active at every call (they are: every call site of
// gj_factor and la_solve sits in wave-uniform control flow of a full wave).
#define SRB_FJ(I) "v_fmac_f64_dpp %" #I ", %" #I ", -%[f] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n\t"
#define SRB_FA(I) "+v"(A[(K + 1 + I) % NZE])
#define SRB_FJ7 SRB_FJ(0) SRB_FJ(1) SRB_FJ(2) SRB_FJ(3) SRB_FJ(4) SRB_FJ(5) SRB_FJ(6)
#define SRB_FJ10 SRB_FJ7 SRB_FJ(7) SRB_FJ(8) SRB_FJ(9)
#define SRB_FJ11 SRB_FJ10 SRB_FJ(10)
#define SRB_FJ15 SRB_FJ11 SRB_FJ(11) SRB_FJ(12) SRB_FJ(13) SRB_FJ(14)
#define SRB_FA7 SRB_FA(0), SRB_FA(1), SRB_FA(2), SRB_FA(3), SRB_FA(4), SRB_FA(5), SRB_FA(6)
#define SRB_FA10 SRB_FA7, SRB_FA(7), SRB_FA(8), SRB_FA(9)
#define SRB_FA11 SRB_FA10, SRB_FA(10)
#define SRB_FA15 SRB_FA11, SRB_FA(11), SRB_FA(12), SRB_FA(13), SRB_FA(14)
#define SRB_FST(N) asm volatile("s_nop 1\n\t" SRB_FJ##N "s_nop 1" : SRB_FA##N : [f] "v"(f), [k] "n"(K))
template <int NZL, int NZE, int K>
__device__ __forceinline__ void gj_fold_step(double (&A)[NZL], double f)
{
    static_assert(NZE == 8 || NZE == 11 || NZE == 12 || NZE == 16, "gj_fold_step: the reduced sizes of the shipped instances");
    if constexpr (NZE == 8) SRB_FST(7);
    else if constexpr (NZE == 11) SRB_FST(10);
    else if constexpr (NZE == 12) SRB_FST(11);
    else SRB_FST(15);
}
#undef SRB_FJ
#undef SRB_FA
#undef SRB_FJ7
#undef SRB_FJ10
#undef SRB_FJ11
#undef SRB_FJ15
#undef SRB_FA7
#undef SRB_FA10
#undef SRB_FA11
#undef SRB_FA15
#undef SRB_FST
template <int NZL, int NZE = NZL>
__device__ __forceinline__ int gj_invert_dpp_fold(double (&A)[NZL], int lane, int regularise)
{
    static_assert(NZL <= 16, "row_newbcast reaches within 16 lanes");
    static_assert(NZE <= NZL, "NZE");
    const int r = lane & 15;
    unsigned long long fail = 0;
    double cs = 1.0;
    srb_static_for(std::make_integer_sequence<int, NZE>{}, [&](auto ic) {
        constexpr int k = decltype(ic)::value;
        double piv = bc16(A[k], k);
        if (regularise && piv <= 1e-14 && piv == piv) piv = 1e-7;
        fail |= __ballot(!(piv > 0.0));
        const double inv = rcp_d(piv);
        const bool me = r == k;
        const double f = me ? 0.0 : A[k] * inv;
        gj_fold_step<NZL, NZE, k>(A, f);
        A[k] = me ? 1.0 : -f;
        cs = me ? inv : cs;
    });
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] *= cs;
    return fail != 0;
}

// The inverse of the solve kernels' reduced Newton matrix: the DPP form where the rows are replicated in every
// 16-lane row of the wave (NZL <= 16 under SRB_USE_DPP, gj_load / mrow), else the readlane form.  With
// row_newbcast as one v_mov_b64_dpp (bc16) the DPP form is the faster one: 2638 against 3114 cycles for
// NZL = 12 (tools/ubench/gj_bench.hip, profiles/factor_chain_ubench.txt), and it holds no pivot row in SGPRs.
// FOLD: the folded form of it (gj_invert_dpp_fold), per instance (srb_dpp_fold, srb_wave.h).
template <int NZL, int NZE = NZL, bool FOLD = srb_dpp_fold(NZL, NZE)>
__device__ __forceinline__ int gj_factor(double (&A)[NZL], int nz, int lane, int regularise)
{
    if constexpr (NZL <= 16 && SRB_USE_DPP) {
        if constexpr (FOLD) return gj_invert_dpp_fold<NZL, NZE>(A, lane, regularise);
        else return gj_invert_dpp<NZL, NZE>(A, lane, regularise);
    } else {
        return gj_invert<NZL, NZE>(A, nz, lane, regularise);
    }
}
