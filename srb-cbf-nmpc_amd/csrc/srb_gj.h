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
// (gj_invert_dpp) where the rows are replicated: 2642 against 3062 cycles for NZL = 12 on MI355X
// (tools/ubench/gj_bench.hip; 3546 while the broadcast still zeroed its destination first).  A step here is
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

// The inverse of the solve kernels' reduced Newton matrix: the DPP form where the rows are replicated in every
// 16-lane row of the wave (NZL <= 16 under SRB_USE_DPP, gj_load / mrow), else the readlane form.  With
// row_newbcast as one v_mov_b64_dpp (bc16) the DPP form is the faster one: 2638 against 3062 cycles for
// NZL = 12 (tools/ubench/gj_bench.hip, profiles/factor_chain_ubench.txt), and it holds no pivot row in SGPRs.
template <int NZL, int NZE = NZL>
__device__ __forceinline__ int gj_factor(double (&A)[NZL], int nz, int lane, int regularise)
{
    if constexpr (NZL <= 16 && SRB_USE_DPP) return gj_invert_dpp<NZL, NZE>(A, lane, regularise);
    else return gj_invert<NZL, NZE>(A, nz, lane, regularise);
}
