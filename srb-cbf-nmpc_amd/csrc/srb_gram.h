// Reduced Gram matrix and right-hand side of the NMPC solve kernel (srb_kernels.hip) over the stored term rows:
// the term-row layout, the obstacle fold, the U / lambda / slack block sums (ul_add, UlLane), gram_rhs and rhs_only.
// Header-only device code, so that tools/ubench/gram_bench.hip times this text and not a copy of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "srb_kernel_params.h"
#include "srb_wave.h"
#include "srb_solve.h"

// --------------------------------------------------------------------------- term rows
// Term row t (Z row of a variable, M_e) at R + t * LDR; LDR = NZL + 1 (odd: lane-parallel row reads stay
// conflict-free).  Rows are zero beyond nz and beyond the count.  Row order: X rows (4N) | CoM-CoP rows |
// U, lambda, slack rows.  Reduced columns: 0 the slack, 1 + j (C - 1) + i the i-th contact-weight dof of
// grid j.
struct TermLayout {
    int N, C, n, nz, E4;
    __device__ __forceinline__ int zr(int v) const { return v < 4 * N ? v : v + E4; }
};

// Obstacle rows, folded per grid (round 5).  Row o = k K + j of grid k is M_o = J_o Z = jx Z_x + jy Z_y - e_s
// (Z_x, Z_y: the stored Z rows 4k, 4k + 2 of the grid's CoM position; OJ[2 o] = jx, OJ[2 o + 1] = jy, set
// by the re-linearisation).  With V_k = [Z_x, Z_y, e_s] and v_o = (jx, jy, -1), the K rows of a grid add
//   sum_j W_o M_o M_o' = V_k S_k V_k',  S_k = sum_j W_o v_o v_o'   and   sum_j CF_o M_o = V_k c_k,  c_k = sum_j CF_o v_o
// to the Gram and the right-hand side: 3 terms a grid instead of K rows (obs_fold forms S_k, c_k; the
// Gram's term (k, u) has A = column u of V_k, B = V_k S_k e_u).  FO holds S_k (00 01 02 11 12 22) and c_k per
// grid, 9 doubles, and a zero entry at grid N for the padding terms.
struct ObsFold {
    const double *OJ;
    double *FO;
    int rO, N, K, NOP;                 // obstacle rows' W / CF offset, grids, rows per grid, 3N padded to 16 NW
    uint64_t mask;                     // NZM = 32: grid-term batches that reach column 16 (all three tiles)
    int rU, C, n;                      // the U, lambda, slack rows (ul_add): first row, contacts, variables
};

// The U, lambda and slack rows [rU, rU + n - 4N) touch only their own grid's C - 1 columns (the slack row
// column 0), so their part of the Gram is block diagonal: H[a][b] += sum_r W_r R[r][a] R[r][b] over the
// 2 + C rows of grid j for a, b in grid j's columns (and W_s at [0][0]), g[a] += sum_r CF_r R[r][a] --
// added directly instead of as MFMA batches of single-entry rows (configs[2] Gram 14 -> 11 batches,
// N = 20 14 + 4 -> 8 + 4).  Lanes tid0, tid0 + step, .. of the caller; after its tile stores.  (One wave with one
// 16 x 16 tile forms the same sums in registers instead, UlLane below.)
template <int NZL, bool GRAM, bool RHS>
__device__ __forceinline__ void ul_add(const double *R, const double *W, const double *CF, const ObsFold &F, double *H,
                                       double *g, int nz, int tid0, int step)
{
    constexpr int LDR = NZL + 1, LDH = NZL + 1;
    const int c1 = F.C - 1, np = F.N * c1 * c1, rl = F.rU + 2 * F.N, rs = F.rU + F.n - 1 - 4 * F.N;
    if (GRAM) {
        for (int e = tid0; e <= np; e += step) {
            if (e == np) { H[0] = H[0] + W[rs]; continue; }  // slack row: Z = e_0
            const int j = e / (c1 * c1), rem = e - j * c1 * c1, a = 1 + j * c1 + rem / c1, b = 1 + j * c1 + rem % c1;
            // the grid's 2 + C rows (C <= 4): every load issued before the first product (predicated, as zo_sum),
            // the sum in the rows' order
            double wv[6], ra[6], rb[6];
#pragma unroll
            for (int u = 0; u < 6; u++) {
                const bool in = u < 2 + F.C;
                const int r = (u < 2) ? F.rU + 2 * j + u : rl + F.C * j + (in ? u - 2 : 0);
                wv[u] = in ? W[r] : 0.0; ra[u] = in ? R[r * LDR + a] : 0.0; rb[u] = in ? R[r * LDR + b] : 0.0;
            }
            const double h0 = H[a * LDH + b];
            __builtin_amdgcn_sched_barrier(0);
            double v = 0.0;
#pragma unroll
            for (int u = 0; u < 6; u++) {
                if (u >= 2 + F.C) break;
                v = fma(wv[u] * ra[u], rb[u], v);
            }
            H[a * LDH + b] = h0 + v;
        }
    }
    if (RHS) {
        for (int a = tid0; a < nz; a += step) {
            if (a == 0) { g[0] += CF[rs]; continue; }
            const int j = (a - 1) / c1;
            double cv[6], ra[6];
#pragma unroll
            for (int u = 0; u < 6; u++) {
                const bool in = u < 2 + F.C;
                const int r = (u < 2) ? F.rU + 2 * j + u : rl + F.C * j + (in ? u - 2 : 0);
                cv[u] = in ? CF[r] : 0.0; ra[u] = in ? R[r * LDR + a] : 0.0;
            }
            const double g0 = g[a];
            __builtin_amdgcn_sched_barrier(0);
            double v = 0.0;
#pragma unroll
            for (int u = 0; u < 6; u++) {
                if (u >= 2 + F.C) break;
                v = fma(cv[u], ra[u], v);
            }
            g[a] = g0 + v;
        }
    }
}

// ul_add's sums formed by the lane that holds the entry in registers (one wave, one 16 x 16 tile: gram_rhs, rhs_only),
// so that the entry is stored once as `accumulator + v` instead of stored, re-read, added to and stored again.  Lane
// (kq, li) of the MFMA D layout holds H[kq + 4 q][li], q = 0 .. 3: of the c1 <= 3 consecutive rows of column li's grid
// block at most one has a & 3 == kq, so a lane forms at most one Gram sum (he; it belongs to register q), the kq = 0
// lane of column li the right-hand-side sum (ge), lane 0 the slack entries W[rs] / CF[rs] (hs).  The sums depend on
// R, W, CF alone: gram_rhs issues load() under the last batch's MFMAs and runs sums() in the accumulator drain (the
// s_nop the hardware wants before the accumulators are read), rhs_only loads ahead of its term rows.  Each sum takes
// ul_add's operands in ul_add's order; lanes without an entry read grid 0's rows (in range) and discard the result.
template <int NZL>
struct UlLane {
    double wv[6], ra[6], rb[6], cv[6], sw, sc;
    int q;
    bool he, ge, hs;
    template <bool GRAM, bool RHS>
    __device__ __forceinline__ void load(const double *R, const double *W, const double *CF, const ObsFold &F, int nz, int lane)
    {
        constexpr int LDR = NZL + 1;
        const int li = lane & 15, kq = lane >> 4;
        const int c1 = F.C - 1, rl = F.rU + 2 * F.N, rs = F.rU + F.n - 1 - 4 * F.N;
        const bool col = li >= 1 && li < nz;
        const int j = col ? (li - 1) / c1 : 0, a0 = 1 + j * c1, off = (kq - a0) & 3;
        he = GRAM && col && off < c1;
        ge = RHS && col && kq == 0;
        hs = lane == 0;
        const int a = he ? a0 + off : 1, b = col ? li : 1;
        q = a >> 2;
#pragma unroll
        for (int u = 0; u < 6; u++) {
            const bool in = u < 2 + F.C;
            const int r = (u < 2) ? F.rU + 2 * j + u : rl + F.C * j + (in ? u - 2 : 0);
            if (GRAM) { wv[u] = W[r]; ra[u] = R[r * LDR + a]; }
            rb[u] = R[r * LDR + b];
            if (RHS) cv[u] = CF[r];
        }
        if (GRAM) sw = W[rs];
        if (RHS) sc = CF[rs];
    }
    template <bool GRAM, bool RHS>
    __device__ __forceinline__ void sums(const ObsFold &F, double &vh, double &vg) const
    {
        vh = 0.0; vg = 0.0;
#pragma unroll
        for (int u = 0; u < 6; u++) {
            if (u >= 2 + F.C) break;
            if (GRAM) vh = fma(wv[u] * ra[u], rb[u], vh);
            if (RHS) vg = fma(cv[u], rb[u], vg);
        }
    }
};

// S_k and c_k (GRAM) or c_k alone into FO: one lane per grid, the K rows in index order
template <bool GRAM>
__device__ __forceinline__ void obs_fold(const double *W, const double *CF, const ObsFold &F, int tid, int NTH)
{
    for (int k = tid; k < F.N; k += NTH) {
        double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
        // the grid's rows in chunks of 8, every load of a chunk issued before the first use (predicated, as
        // zo_sum): one LDS round trip a chunk instead of one a row; the sums keep the row order
        for (int j0 = 0; j0 < F.K; j0 += 8) {
            double cfv[8], jxv[8], jyv[8], wv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bool in = j0 + u < F.K;
                const int o = k * F.K + (in ? j0 + u : 0);
                cfv[u] = in ? CF[F.rO + o] : 0.0; jxv[u] = in ? F.OJ[2 * o] : 0.0; jyv[u] = in ? F.OJ[2 * o + 1] : 0.0;
                wv[u] = (GRAM && in) ? W[F.rO + o] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (j0 + u >= F.K) break;
                const double cf = cfv[u], jx = jxv[u], jy = jyv[u];
                c0 = fma(cf, jx, c0); c1 = fma(cf, jy, c1); c2 -= cf;
                if (GRAM) {
                    const double w = wv[u], wx = w * jx, wy = w * jy;
                    s00 = fma(wx, jx, s00); s01 = fma(wx, jy, s01); s02 -= wx; s11 = fma(wy, jy, s11); s12 -= wy; s22 += w;
                }
            }
        }
        double *f = F.FO + 9 * k;
        if (GRAM) { f[0] = s00; f[1] = s01; f[2] = s02; f[3] = s11; f[4] = s12; f[5] = s22; }
        f[6] = c0; f[7] = c1; f[8] = c2;
    }
}

// Highest reduced column term row t (t < rO) touches: X rows of grid k reach grid k, a CoM-CoP row of grid i
// grid i + 1, U / lambda rows their own grid.  With NZM = 32 a batch of 16 terms whose rows all stop below
// column 16 needs the (0,0) tile only (gram_rhs, rhs_only; `bmask` bit b = batch b needs all three; the
// obstacle grid terms likewise in ObsFold::mask).
__device__ __forceinline__ int term_maxcol(int t, int N, int C, int n, int rC, int NE, int rU)
{
    const int c1 = C - 1;
    if (t < rC) return (t / 4 + 1) * c1;
    if (t < rC + NE) return ((t - rC) / 2 + 2) * c1;
    if (t < rU) return 0;
    const int v = 4 * N + (t - rU);
    if (v < 6 * N) return ((v - 4 * N) / 2 + 1) * c1;
    if (v < n - 1) return ((v - 6 * N) / C + 1) * c1;
    return 0;                                                    // slack row (column 0), padding
}

template <int NZM>
__device__ __forceinline__ uint64_t full_batches(int rO, int N, int C, int n, int rC, int NE, int rU, int lane)
{
    if constexpr (NZM == 16) return ~0ull;
    int f = 0;
    if (16 * lane < rO) {
        int mx = 0;
        for (int u = 0; u < 16; u++) mx = max(mx, term_maxcol(16 * lane + u, N, C, n, rC, NE, rU));
        f = mx >= 16;
    }
    return __ballot(f) | ((rO > 16 * 64) ? (1ull << 63) : 0ull);   /* (more than 64 batches: the last bit covers the rest) */
}

template <int NZM>
__device__ __forceinline__ uint64_t full_obs_batches(int N, int C, int NOP, int lane)
{
    if constexpr (NZM == 16) return ~0ull;
    const int kmax = min((16 * lane + 15) / 3, N - 1);
    return __ballot(16 * lane < NOP && (kmax + 1) * (C - 1) >= 16) | ((NOP > 16 * 64) ? (1ull << 63) : 0ull);
}

__device__ __forceinline__ bool batch_full(uint64_t bmask, int t0)
{
    const int b = t0 >> 4;
    return (bmask >> (b < 63 ? b : 63)) & 1ull;
}

// element `col` of stored term row r
template <int NZL>
__device__ __forceinline__ double term_elem(const double *R, int r, int col)
{
    constexpr int LDR = NZL + 1;
    if constexpr (NZL <= 16) {
        // one column block: the load is unconditional (the column clamped into the row), the padding columns
        // selected to zero -- a plain ds_read and a v_cndmask instead of an exec-mask block per load
        const double v = R[r * LDR + min(col, NZL - 1)];
        return (col < NZL) ? v : 0.0;
    } else {
        // two column blocks (N = 20): measured slower with the unconditional form (config 5 +0.5 %), kept predicated
        return (col < NZL) ? R[r * LDR + col] : 0.0;
    }
}

// obstacle grid term t = 3 k + u: A element (column u of V_k) for column col, and the row of S_k / entry of
// c_k it pairs with (padding terms: grid N, all zero)
template <int NZL>
__device__ __forceinline__ double obs_term_a(const double *R, const ObsFold &F, int t, int col, double &zx, double &zy)
{
    constexpr int LDR = NZL + 1;
    const int k = t / 3, u = t - 3 * k, xr = 4 * min(k, F.N - 1);
    zx = (col < NZL) ? R[xr * LDR + col] : 0.0;
    zy = (col < NZL) ? R[(xr + 2) * LDR + col] : 0.0;
    const double es = (col == 0) ? 1.0 : 0.0;
    return (u == 0) ? zx : (u == 1) ? zy : es;
}

// GRAM: H = sum_t W_t r_t r_t' over the stored term rows [0, cnt) plus the folded obstacle grid terms
//   [0, NOP) (when nko > 0, the NLP stage): v_mfma_f64_16x16x4f64 with A[a][k] = r_{t0+k}[a],
//   B[k][b] = W_{t0+k} r_{t0+k}[b] (grid terms: B = V_k S_k e_u); lane l supplies term t0 + (l >> 4),
//   column l & 15; D layout row (l >> 4) + 4 q, column l & 15; NZM = 32: tiles (0,0), (0,1), (1,1).  Four
//   term groups per batch: every operand load of the batch issues before the first MFMA waits on one; with one
//   column block (NZM = 16) the loads of batch b + 1 issue before the MFMAs of batch b.
// RHS: g[a] = sum_t CF_t r_t[a]: the very element lane l forms for the MFMA is the one its (column, term)
//   pair needs, so the right-hand side costs one FMA per element; the four term chunks combine by permlane
//   swaps.
// cnt and NOP are multiples of 16 NW; W / CF are zero beyond every real row.
// NW > 1: wave w takes the w-th NW-th of both ranges; the per-wave partial tiles / right-hand sides are
// summed through LDS (`part`: NW x NT x 256 + NW x NZM doubles).
//
// Vector form (gram_rhs_vec below; the callers choose it for one wave, one column block, NZL <= 12 and the shape
// compiled in, SH -- a function of its own, so that every other instance instantiates the gram_rhs it always did): the fp64
// MFMA executes 16 x 16 x 4 multiply-adds per 4 terms of which a symmetric nz x nz matrix needs a quarter, at the
// same peak rate as the vector ALU, so the accumulation runs on the vector ALU instead.  Lane (kq, li) loads the same
// element a = r_{t0 + 4u + kq}[li] (same loads, same look-ahead buffers), forms wa = w a once, and adds
// bcast_j(a) wa to private accumulators hv[j] (bcast_j: lane j of this lane's 16-lane row): hv[j] of lane (kq, li)
// is the partial H[j][li] over the terms of row kq.  The batch sequence is unrolled, so the group (batch, u) is known
// when the kernel is compiled, and with it the highest column its four term rows reach (GramShape::ncols: a state
// row of grid k depends on the dofs of grids <= k only): accumulators above it are left out of the group, the dropped
// terms being 0 x finite products.  The select of the padding columns is dropped too: lanes li >= NZL carry column
// NZL - 1 again and are never stored, lanes nz <= li < NZL read the rows' zeros.  After the last batch a
// reduce-scatter by permlane swaps (gram_scatter) sums the four rows and leaves lane (kq, li) with H[kq + 4q][li],
// q < 3, the MFMA's D layout, so the UlLane sums and the stores below are the same for both forms.  The sum over the
// terms is associated by term row (four partial sums), not in the MFMA's order: H differs from the MFMA form's in
// its last bits.  g is formed exactly as before.
//   SRB_GRAM_DPP_ASM: one v_fmac_f64_dpp row_newbcast:j per accumulator (gram_group; the compiler does not fold the
//     broadcast into the FMA, so this is inline assembly -- see the wait states there);
//   SRB_GRAM_DPP_MOV: bc16() + fma(), v_mov_b64_dpp + v_fmac_f64, no assembly.
#define SRB_GRAM_MFMA 0
#define SRB_GRAM_DPP_ASM 1
#define SRB_GRAM_DPP_MOV 2
#ifndef SRB_GRAM_FORM
#define SRB_GRAM_FORM SRB_GRAM_DPP_ASM
#endif

// The term rows of a compiled shape (N grids, C contacts, K obstacle rows a grid; all 0: a run-time shape) at one wave
// per agent, as nmpc_agent lays them out: 4N state rows, 2 (N - 1) CoM-CoP rows, padding to RU; NK obstacle rows
// padded to NKP.  Batch b < NB1 holds the rows 16 b .. 16 b + 15, batch NB1 + i the obstacle rows 16 i .. 16 i + 15.
template <int N_, int C_, int K_>
struct GramShape {
    static constexpr int N = N_, C = C_, K = K_;
    static constexpr int RC = 4 * N, NE = 2 * (N - 1), RU = (RC + NE + 15) / 16 * 16, NK = N * K, NKP = (NK + 15) / 16 * 16;
    static constexpr int NB1 = RU / 16, NBO = NKP / 16, NZ = N * (C - 1) + 1;
    // the columns [0, ncols) hold every non-zero of the four term rows of group u of batch b: term_maxcol's rule for the
    // stored rows; obstacle row o of grid o / K is jx Z_x + jy Z_y - e_s of that grid's state rows.  Padding rows: 0.
    static constexpr int ncols(int b, int u)
    {
        int mx = 0;
        for (int k = 0; k < 4; k++) {
            const int t = 16 * (b < NB1 ? b : b - NB1) + 4 * u + k;
            const int g = (b < NB1) ? (t < RC ? t / 4 + 1 : t < RC + NE ? (t - RC) / 2 + 2 : 0) : (t < NK ? t / K + 1 : 0);
            mx = g > mx ? g : mx;
        }
        return mx == 0 ? 0 : mx * (C - 1) + 1;
    }
};

// hv[j] += bcast_j(a) wa, j < NCOL.  The assembly form is one statement a group, so that the compiler cannot move or
// copy an operand between its instructions.  Wait states: the DPP operand `a` needs two wait states after a VALU write
// of it (a v_accvgpr_read un-spill, a copy); the compiler neither sees the DPP read inside the string nor pads it,
// and a missing pad gives wrong values with no message, so every statement opens with its own s_nop 1.  Only `a` is
// DPP-read; wa and the accumulators are ordinary VALU operands (interlocked).  Operands are "v": the solve kernel
// parks spills in AGPRs, which a DPP instruction cannot name.
#define SRB_GFM(J) "v_fmac_f64_dpp %" #J ", %[a], %[wa] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define SRB_GAC(J) "+v"(hv[J])
#define SRB_GST(S, ...) asm volatile("s_nop 1\n\t" S : __VA_ARGS__ : [a] "v"(a), [wa] "v"(wa))
#define SRB_GF4 SRB_GFM(0) SRB_GFM(1) SRB_GFM(2) SRB_GFM(3)
#define SRB_GF8 SRB_GF4 SRB_GFM(4) SRB_GFM(5) SRB_GFM(6) SRB_GFM(7)
#define SRB_GA4 SRB_GAC(0), SRB_GAC(1), SRB_GAC(2), SRB_GAC(3)
#define SRB_GA8 SRB_GA4, SRB_GAC(4), SRB_GAC(5), SRB_GAC(6), SRB_GAC(7)
template <int NCOL, int FORM>
__device__ __forceinline__ void gram_group(double (&hv)[12], double a, double wa)
{
    static_assert(NCOL >= 0 && NCOL <= 12, "gram_group: NCOL");
    if constexpr (FORM == SRB_GRAM_DPP_ASM) {
        if constexpr (NCOL == 1) SRB_GST(SRB_GFM(0), SRB_GAC(0));
        else if constexpr (NCOL == 2) SRB_GST(SRB_GFM(0) SRB_GFM(1), SRB_GAC(0), SRB_GAC(1));
        else if constexpr (NCOL == 3) SRB_GST(SRB_GFM(0) SRB_GFM(1) SRB_GFM(2), SRB_GAC(0), SRB_GAC(1), SRB_GAC(2));
        else if constexpr (NCOL == 4) SRB_GST(SRB_GF4, SRB_GA4);
        else if constexpr (NCOL == 5) SRB_GST(SRB_GF4 SRB_GFM(4), SRB_GA4, SRB_GAC(4));
        else if constexpr (NCOL == 6) SRB_GST(SRB_GF4 SRB_GFM(4) SRB_GFM(5), SRB_GA4, SRB_GAC(4), SRB_GAC(5));
        else if constexpr (NCOL == 7) SRB_GST(SRB_GF4 SRB_GFM(4) SRB_GFM(5) SRB_GFM(6), SRB_GA4, SRB_GAC(4), SRB_GAC(5), SRB_GAC(6));
        else if constexpr (NCOL == 8) SRB_GST(SRB_GF8, SRB_GA8);
        else if constexpr (NCOL == 9) SRB_GST(SRB_GF8 SRB_GFM(8), SRB_GA8, SRB_GAC(8));
        else if constexpr (NCOL == 10) SRB_GST(SRB_GF8 SRB_GFM(8) SRB_GFM(9), SRB_GA8, SRB_GAC(8), SRB_GAC(9));
        else if constexpr (NCOL == 11) SRB_GST(SRB_GF8 SRB_GFM(8) SRB_GFM(9) SRB_GFM(10), SRB_GA8, SRB_GAC(8), SRB_GAC(9), SRB_GAC(10));
        else if constexpr (NCOL == 12)
            SRB_GST(SRB_GF8 SRB_GFM(8) SRB_GFM(9) SRB_GFM(10) SRB_GFM(11), SRB_GA8, SRB_GAC(8), SRB_GAC(9), SRB_GAC(10), SRB_GAC(11));
    } else {
#pragma unroll
        for (int j = 0; j < NCOL; j++) hv[j] = fma(bc16(a, j), wa, hv[j]);
    }
}
#undef SRB_GFM
#undef SRB_GAC
#undef SRB_GST
#undef SRB_GF4
#undef SRB_GF8
#undef SRB_GA4
#undef SRB_GA8

// the four groups of batch B: the right-hand side's FMA as in the MFMA form, then the group's accumulators
template <class SH, int FORM, bool RHS, int B>
__device__ __forceinline__ void gram_batch(double (&hv)[12], double &ps, const double (&ar)[4], const double (&w)[4],
                                           const double (&c)[4])
{
#define SRB_GG(U) { const double a = ar[U]; if (RHS) ps = fma(c[U], a, ps); gram_group<SH::ncols(B, U), FORM>(hv, a, w[U] * a); }
    SRB_GG(0) SRB_GG(1) SRB_GG(2) SRB_GG(3)
#undef SRB_GG
}
// (srb_static_for: srb_wave.h)

// {x over lanes l and l ^ 32 summed} in lanes 0 .. 31, {y likewise} in lanes 32 .. 63: v_permlane32_swap exchanges
// lanes 32 .. 63 of its first operand with lanes 0 .. 31 of its second; W = 16 the same over the 16-lane rows
// (v_permlane16_swap: the odd rows of the first with the even rows of the second): x in the even rows, y in the odd
template <int W>
__device__ __forceinline__ double swap_sum2(double x, double y)
{
    const unsigned long long ux = (unsigned long long)__double_as_longlong(x), uy = (unsigned long long)__double_as_longlong(y);
    const unsigned xl = (unsigned)ux, xh = (unsigned)(ux >> 32), yl = (unsigned)uy, yh = (unsigned)(uy >> 32);
    auto l = (W == 16) ? __builtin_amdgcn_permlane16_swap(xl, yl, false, false) : __builtin_amdgcn_permlane32_swap(xl, yl, false, false);
    auto h = (W == 16) ? __builtin_amdgcn_permlane16_swap(xh, yh, false, false) : __builtin_amdgcn_permlane32_swap(xh, yh, false, false);
    return __longlong_as_double((long long)(((unsigned long long)h[0] << 32) | l[0])) +
           __longlong_as_double((long long)(((unsigned long long)h[1] << 32) | l[1]));
}
// The four 16-lane rows' partial sums hv[j] (accumulators j >= NZE: zero) summed and scattered: lane (kq, li) gets
// H[kq + 4q][li] in d[q].  Stage 1 pairs j with j + 2 across the wave's halves (rows 0, 1 keep j, rows 2, 3 j + 2),
// stage 2 pairs j with j + 1 across neighbouring rows: 9 swaps of a pair where 12 butterflies took 24, each sum
// (p_0 + p_2) + (p_1 + p_3) over the rows' partials as chunk_sum16 forms it.  The stages are interleaved across the
// accumulators (every swap of a stage before the first add that waits on one).
__device__ __forceinline__ d4 gram_scatter(const double (&hv)[12])
{
    double t[6];
#pragma unroll
    for (int m = 0; m < 6; m++) {
        const int j = 4 * (m >> 1) + (m & 1);
        t[m] = swap_sum2<32>(hv[j], hv[j + 2]);
    }
    d4 d;
#pragma unroll
    for (int q = 0; q < 3; q++) d[q] = swap_sum2<16>(t[2 * q], t[2 * q + 1]);
    d[3] = 0.0;
    return d;
}

// gram_rhs in the vector form: one wave, the batch sequence of the compiled shape SH unrolled (SH::NB1 row batches,
// then with nko > 0 SH::NBO obstacle batches from row F.rO), batch b in operand buffer b & 1, the loads of the batch
// after it -- or, under the last batch, the UlLane operands -- issued first.  Loads, the right-hand side and the
// stores are gram_rhs's one-wave, one-tile ones.
template <int NZL, bool RHS, class SH, int FORM>
__device__ __forceinline__ void gram_rhs_vec(const double *R, const double *W, const double *CF, const ObsFold &F, int nko,
                                             double *H, double *g, int nz, int lane)
{
    constexpr int LDH = NZL + 1;
    const int li = lane & 15, kq = lane >> 4;
    double hv[12], ps = 0.0;
#pragma unroll
    for (int j = 0; j < 12; j++) hv[j] = 0.0;
    UlLane<NZL> ul;
    double ulh = 0.0, ulg = 0.0;
    auto loadb = [&](int t0, double (&a)[4], double (&w)[4], double (&c)[4]) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = t0 + 4 * u + kq;
            a[u] = R[r * (NZL + 1) + min(li, NZL - 1)];          // no padding select: lanes li >= NZL are never stored
            w[u] = W[r];
            c[u] = RHS ? CF[r] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);         // the next batch's loads stay ahead of this batch's accumulation
    };
    auto ulload = [&]() { ul.template load<true, RHS>(R, W, CF, F, nz, lane); __builtin_amdgcn_sched_barrier(0); };
    double ab[2][4], wb[2][4], cb[2][4];
    const bool obs = nko > 0;
    loadb(0, ab[0], wb[0], cb[0]);
    srb_static_for(std::make_integer_sequence<int, SH::NB1>{}, [&](auto ic) {
        constexpr int b = decltype(ic)::value, cu = b & 1, nx = cu ^ 1;
        if constexpr (b + 1 < SH::NB1) {
            loadb(16 * (b + 1), ab[nx], wb[nx], cb[nx]);
        } else {
            if (obs) loadb(F.rO, ab[nx], wb[nx], cb[nx]);
            else ulload();
        }
        gram_batch<SH, FORM, RHS, b>(hv, ps, ab[cu], wb[cu], cb[cu]);
        __builtin_amdgcn_sched_barrier(0);
    });
    if (obs)
        srb_static_for(std::make_integer_sequence<int, SH::NBO>{}, [&](auto ic) {
            constexpr int i = decltype(ic)::value, b = SH::NB1 + i, cu = b & 1, nx = cu ^ 1;
            if constexpr (i + 1 < SH::NBO) loadb(F.rO + 16 * (i + 1), ab[nx], wb[nx], cb[nx]);
            else ulload();
            gram_batch<SH, FORM, RHS, b>(hv, ps, ab[cu], wb[cu], cb[cu]);
            __builtin_amdgcn_sched_barrier(0);
        });
    // the accumulators were last written inside an assembly string, which the compiler pads for nothing: the two wait
    // states a v_permlane*_swap wants after a VALU write of its operand
    if constexpr (FORM == SRB_GRAM_DPP_ASM)
        asm volatile("s_nop 1" : "+v"(hv[0]), "+v"(hv[1]), "+v"(hv[2]), "+v"(hv[3]), "+v"(hv[4]), "+v"(hv[5]), "+v"(hv[6]),
                     "+v"(hv[7]), "+v"(hv[8]), "+v"(hv[9]), "+v"(hv[10]), "+v"(hv[11]));
    const d4 acc = gram_scatter(hv);
    ul.template sums<true, RHS>(F, ulh, ulg);
    if (RHS) {
        const double gs = chunk_sum16(ps);
        if (kq == 0 && li < nz) g[li] = ul.ge ? gs + ulg : ul.hs ? gs + ul.sc : gs;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = kq + 4 * q;
        const double h = acc[q];
        if (r < NZL && li < NZL) H[r * LDH + li] = (ul.he && q == ul.q) ? h + ulh : (ul.hs && q == 0) ? h + ul.sw : h;
    }
}

template <int NZL, bool RHS, int NW>
__device__ __forceinline__ void gram_rhs(const double *R, const double *W, const double *CF, int cnt, const ObsFold &F,
                                         int nko, double *H, double *g, int nz, int tid, double *part, uint64_t bmask)
{
    constexpr int NZM = ((NZL + 15) / 16) * 16;
    constexpr int LDH = NZL + 1;            // H holds rows / columns < NZL only (the rest of the tiles are 0)
    constexpr int NT = (NZM == 16) ? 1 : 3, NTC = NZM / 16;
    const int lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    constexpr bool FOLD = !SRB_OBS_STORED(NZL);
    if (FOLD && nko > 0) {
        obs_fold<true>(W, CF, F, tid, 64 * NW);
        srb_sync<NW>();
    }
    d4 acc[NT];
    double ps[NTC];
    // one wave, one tile: the U / lambda / slack sums join the accumulators in registers (UlLane), no ul_add pass
    constexpr bool ULF = NZM == 16 && NW == 1;
    UlLane<NZL> ul;
    double ulh = 0.0, ulg = 0.0;
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < NTC; t++) ps[t] = 0.0;
    // FULL: all NTC column blocks; otherwise block 0 only (every row of the batch is zero beyond column 15)
    auto body = [&](int t0, auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;
        constexpr int NB = FULL ? NTC : 1;
        double a[4][NTC], w[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = t0 + 4 * u + kq;
#pragma unroll
            for (int tc = 0; tc < NB; tc++) a[u][tc] = term_elem<NZL>(R, r, 16 * tc + li);
            w[u] = W[r];
            c[u] = RHS ? CF[r] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);     // keep the batch's loads ahead of its MFMAs
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (RHS)
#pragma unroll
                for (int tc = 0; tc < NB; tc++) ps[tc] = fma(c[u], a[u][tc], ps[tc]);
            if constexpr (NZM == 16 || !FULL) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], w[u] * a[u][0], acc[0], 0, 0, 0);
            } else {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], w[u] * a[u][0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], w[u] * a[u][NTC - 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][NTC - 1], w[u] * a[u][NTC - 1], acc[2], 0, 0, 0);
            }
        }
    };
    // folded obstacle grid terms t0 .. t0 + 15
    auto obody = [&](int t0, auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;
        constexpr int NB = FULL ? NTC : 1;
        double a[4][NTC], b[4][NTC], c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 4 * u + kq, k = t / 3, uu = t - 3 * k;
            const double *f = F.FO + 9 * min(k, F.N);
            const int i1 = (uu == 0) ? 1 : (uu == 1) ? 3 : 4, i2 = (uu == 0) ? 2 : (uu == 1) ? 4 : 5;
            const double s0 = f[uu], s1 = f[i1], s2 = f[i2];
            c[u] = RHS ? f[6 + uu] : 0.0;
#pragma unroll
            for (int tc = 0; tc < NB; tc++) {
                double zx, zy;
                a[u][tc] = obs_term_a<NZL>(R, F, t, 16 * tc + li, zx, zy);
                b[u][tc] = fma(s0, zx, fma(s1, zy, (16 * tc + li == 0) ? s2 : 0.0));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (RHS)
#pragma unroll
                for (int tc = 0; tc < NB; tc++) ps[tc] = fma(c[u], a[u][tc], ps[tc]);
            if constexpr (NZM == 16 || !FULL) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], b[u][0], acc[0], 0, 0, 0);
            } else {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], b[u][0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][0], b[u][NTC - 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][NTC - 1], b[u][NTC - 1], acc[2], 0, 0, 0);
            }
        }
    };
    if constexpr (NZM == 16) {
        // One column block, stored obstacle rows: the wave's batches -- its chunk of the term rows, then (nko > 0)
        // its chunk of the obstacle rows -- as one sequence, the operand loads of batch i + 1 issued before the
        // MFMAs of batch i (two operand buffers, the loop unrolled by two with the buffers swapped; the first batch
        // loaded ahead of the loop, the last one peeled: nothing is read beyond the wave's own ranges, and with
        // nko = 0 nothing of the obstacle range).  Every accumulator takes the same operands in the same order as
        // in the one-batch-at-a-time loop below.
        const int chunk = cnt / NW, tb = wv * chunk, och = nko / NW, ob = F.rO + wv * och;
        const int nb1 = chunk >> 4, nbt = nb1 + (och >> 4);
        auto bt0 = [&](int i) { return i < nb1 ? tb + 16 * i : ob + 16 * (i - nb1); };
        auto loadb = [&](int t0, double (&a)[4], double (&w)[4], double (&c)[4]) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = t0 + 4 * u + kq;
                a[u] = R[r * (NZL + 1) + min(li, NZL - 1)];      // term_elem's load; its select waits in mmb
                w[u] = W[r];
                c[u] = RHS ? CF[r] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);     // the next batch's loads stay ahead of this batch's MFMAs
        };
        auto mmb = [&](const double (&ar)[4], const double (&w)[4], const double (&c)[4]) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double a = (li < NZL) ? ar[u] : 0.0;
                if (RHS) ps[0] = fma(c[u], a, ps[0]);
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w[u] * a, acc[0], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        if (nbt > 0) {
            double a0[4], w0[4], c0[4], a1[4], w1[4], c1[4];
            loadb(bt0(0), a0, w0, c0);
            int i = 0;
#pragma clang loop unroll(disable)
            for (; i + 2 < nbt; i += 2) {
                loadb(bt0(i + 1), a1, w1, c1);
                mmb(a0, w0, c0);
                loadb(bt0(i + 2), a0, w0, c0);
                mmb(a1, w1, c1);
            }
            if (i + 1 < nbt) {
                loadb(bt0(i + 1), a1, w1, c1);
                mmb(a0, w0, c0);
                if constexpr (ULF) { ul.template load<true, RHS>(R, W, CF, F, nz, lane); __builtin_amdgcn_sched_barrier(0); }
                mmb(a1, w1, c1);
            } else {
                if constexpr (ULF) { ul.template load<true, RHS>(R, W, CF, F, nz, lane); __builtin_amdgcn_sched_barrier(0); }
                mmb(a0, w0, c0);
            }
        } else if constexpr (ULF) {
            ul.template load<true, RHS>(R, W, CF, F, nz, lane);
        }
        if constexpr (ULF) ul.template sums<true, RHS>(F, ulh, ulg);       // in the accumulator drain
    } else {
        // NZM = 32 with several waves: the batches dealt round-robin over the waves (the full-width ones
        // cluster at high grids, so contiguous halves left one wave with most of them); else contiguous
        constexpr bool ILV = NZM == 32 && NW > 1;
        const int chunk = cnt / NW, tb = ILV ? 16 * wv : wv * chunk, te = ILV ? cnt : tb + chunk, ts = ILV ? 16 * NW : 16;
#pragma clang loop unroll(disable)
        for (int t0 = tb; t0 < te; t0 += ts) {
            if (NZM == 16 || batch_full(bmask, t0)) body(t0, std::integral_constant<bool, true>{});
            else body(t0, std::integral_constant<bool, false>{});
        }
        if (FOLD && nko > 0) {
            const int och = F.NOP / NW, ob = ILV ? 16 * wv : wv * och, oe = ILV ? F.NOP : ob + och;
#pragma clang loop unroll(disable)
            for (int t0 = ob; t0 < oe; t0 += ts) {
                if (NZM == 16 || batch_full(F.mask, t0)) obody(t0, std::integral_constant<bool, true>{});
                else obody(t0, std::integral_constant<bool, false>{});
            }
        } else if (nko > 0) {                       // stored obstacle rows [rO, rO + nko)
            const int och = nko / NW, ob = F.rO + wv * och;
#pragma clang loop unroll(disable)
            for (int t0 = ob; t0 < ob + och; t0 += 16) body(t0, std::integral_constant<bool, true>{});
        }
    }
    double gs[NTC];
    if (RHS)
#pragma unroll
        for (int tc = 0; tc < NTC; tc++) gs[tc] = chunk_sum16(ps[tc]);
    if constexpr (NW <= 2) {
        // wave 0 stores its tiles; with two waves, wave 1 then adds its own in place (a fixed
        // order: bit-reproducible, and no partial-Gram scratch in LDS)
        auto put = [&](int i, int j, double v, bool add) {
            if (i < NZL && j < NZL) H[i * LDH + j] = add ? H[i * LDH + j] + v : v;
        };
#pragma unroll
        for (int ph = 0; ph < NW; ph++) {
            if (ph > 0) __syncthreads();
            if (wv == ph) {
                if (RHS)
#pragma unroll
                    for (int tc = 0; tc < NTC; tc++)
                        if (kq == 0 && 16 * tc + li < nz) {
                            if constexpr (ULF) g[li] = ul.ge ? gs[0] + ulg : ul.hs ? gs[0] + ul.sc : gs[0];
                            else g[16 * tc + li] = ph ? g[16 * tc + li] + gs[tc] : gs[tc];
                        }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int r = kq + 4 * q;
                    if constexpr (ULF) {
                        const double h = acc[0][q];
                        put(r, li, (ul.he && q == ul.q) ? h + ulh : (ul.hs && q == 0) ? h + ul.sw : h, false);
                        continue;
                    }
                    put(r, li, acc[0][q], ph > 0);
                    if constexpr (NZM == 32) {
                        put(r, 16 + li, acc[1][q], ph > 0);
                        put(16 + li, r, acc[1][q], ph > 0);
                        put(16 + r, 16 + li, acc[2][q], ph > 0);
                    }
                }
                if (ph == NW - 1 && !ULF) ul_add<NZL, true, RHS>(R, W, CF, F, H, g, nz, lane, 64);   /* (same wave, after its stores) */
            }
        }
    } else {
        double *pg = part + NW * NT * 256;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) part[((wv * NT + t) * 4 + q) * 64 + lane] = acc[t][q];
        if (RHS)
#pragma unroll
            for (int tc = 0; tc < NTC; tc++)
                if (kq == 0) pg[wv * NZM + 16 * tc + li] = gs[tc];
        __syncthreads();
        for (int e = tid; e < NT * 256; e += 64 * NW) {
            const int t = e >> 8, q = (e >> 6) & 3, ln = e & 63;
            double v = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) v += part[((w2 * NT + t) * 4 + q) * 64 + ln];
            const int r = (ln >> 4) + 4 * q, cl = ln & 15;
            if (t == 0) { if (r < NZL && cl < NZL) H[r * LDH + cl] = v; }
            else if (t == 1) { if (16 + cl < NZL) { H[r * LDH + 16 + cl] = v; H[(16 + cl) * LDH + r] = v; } }
            else if (16 + r < NZL && 16 + cl < NZL) H[(16 + r) * LDH + 16 + cl] = v;
        }
        if (RHS && tid < nz) {
            double v = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) v += pg[w2 * NZM + tid];
            g[tid] = v;
        }
        __syncthreads();
        ul_add<NZL, true, RHS>(R, W, CF, F, H, g, nz, tid, 64 * NW);
    }
}

// g[a] = sum_t CF_t r_t[a] alone (corrector): same lane mapping and term ranges as gram_rhs (c_k refolded,
// S_k kept), eight term groups per batch so that 16 loads are in flight before the FMAs need them.
template <int NZL, int NW>
__device__ __forceinline__ void rhs_only(const double *R, const double *CF, int cnt, const ObsFold &F, int nko, double *g,
                                         int nz, int tid, double *part, uint64_t bmask)
{
    constexpr int NZM = ((NZL + 15) / 16) * 16;
    constexpr int NTC = NZM / 16;
    const int lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    constexpr bool FOLD = !SRB_OBS_STORED(NZL);
    if (FOLD && nko > 0) {
        obs_fold<false>(nullptr, CF, F, tid, 64 * NW);
        srb_sync<NW>();
    }
    double ps[2][NTC];
    constexpr bool ULF = NZM == 16 && NW == 1;     // as gram_rhs: the U / lambda / slack sum joins sv in registers
    UlLane<NZL> ul;
    double ulh = 0.0, ulg = 0.0;
#pragma unroll
    for (int t = 0; t < NTC; t++) { ps[0][t] = 0.0; ps[1][t] = 0.0; }
    auto chunk32 = [&](int t0, auto fullc) {
        constexpr int NB = decltype(fullc)::value ? NTC : 1;
        double a[8][NTC], c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int r = t0 + 4 * u + kq;
            c[u] = CF[r];
#pragma unroll
            for (int tc = 0; tc < NB; tc++) a[u][tc] = term_elem<NZL>(R, r, 16 * tc + li);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
            for (int tc = 0; tc < NB; tc++) ps[u & 1][tc] = fma(c[u], a[u][tc], ps[u & 1][tc]);
    };
    auto schunk16 = [&](int t0, auto fullc) {          // stored rows t0 .. t0 + 15
        constexpr int NB = decltype(fullc)::value ? NTC : 1;
        double a[4][NTC], c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = t0 + 4 * u + kq;
            c[u] = CF[r];
#pragma unroll
            for (int tc = 0; tc < NB; tc++) a[u][tc] = term_elem<NZL>(R, r, 16 * tc + li);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int tc = 0; tc < NB; tc++) ps[u & 1][tc] = fma(c[u], a[u][tc], ps[u & 1][tc]);
    };
    auto ochunk16 = [&](int t0, auto fullc) {
        constexpr int NB = decltype(fullc)::value ? NTC : 1;
        double a[4][NTC], c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 4 * u + kq, k = t / 3, uu = t - 3 * k;
            c[u] = F.FO[9 * min(k, F.N) + 6 + uu];
#pragma unroll
            for (int tc = 0; tc < NB; tc++) {
                double zx, zy;
                a[u][tc] = obs_term_a<NZL>(R, F, t, 16 * tc + li, zx, zy);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int tc = 0; tc < NB; tc++) ps[u & 1][tc] = fma(c[u], a[u][tc], ps[u & 1][tc]);
    };
    auto range = [&](int tb, int te, bool st) {     // stored rows [tb, te) (st: the stored obstacle rows)
        int t0 = tb;
#pragma clang loop unroll(disable)
        for (; t0 + 32 <= te; t0 += 32) {
            if (NZM == 16 || st || batch_full(bmask, t0) || batch_full(bmask, t0 + 16))
                chunk32(t0, std::integral_constant<bool, true>{});
            else
                chunk32(t0, std::integral_constant<bool, false>{});
        }
#pragma clang loop unroll(disable)
        for (; t0 < te; t0 += 4) {
            const int r = t0 + kq;
            const double cc = CF[r];
#pragma unroll
            for (int tc = 0; tc < NTC; tc++) ps[0][tc] = fma(cc, term_elem<NZL>(R, r, 16 * tc + li), ps[0][tc]);
        }
    };
    if constexpr (ULF) ul.template load<false, true>(R, nullptr, CF, F, nz, lane);     // ahead of the term rows' loads
    {
        constexpr bool ILV = NZM == 32 && NW > 1;       // batches round-robin over the waves, as gram_rhs
        const int chunk = cnt / NW, tb = wv * chunk;
        if constexpr (ILV) {
#pragma clang loop unroll(disable)
            for (int t0 = 16 * wv; t0 < cnt; t0 += 16 * NW) {
                if (batch_full(bmask, t0)) schunk16(t0, std::integral_constant<bool, true>{});
                else schunk16(t0, std::integral_constant<bool, false>{});
            }
        } else {
            range(tb, tb + chunk, false);
        }
        if (!FOLD && nko > 0) {
            const int och = nko / NW, ob = F.rO + wv * och;
            range(ob, ob + och, true);
        }
        if (FOLD && nko > 0) {
            const int och = F.NOP / NW, ob = ILV ? 16 * wv : wv * och, oe = ILV ? F.NOP : ob + och, os = ILV ? 16 * NW : 16;
#pragma clang loop unroll(disable)
            for (int o0 = ob; o0 < oe; o0 += os) {
                if (NZM == 16 || batch_full(F.mask, o0)) ochunk16(o0, std::integral_constant<bool, true>{});
                else ochunk16(o0, std::integral_constant<bool, false>{});
            }
        }
    }
    if constexpr (ULF) ul.template sums<false, true>(F, ulh, ulg);
    double sv[NTC];
#pragma unroll
    for (int tc = 0; tc < NTC; tc++) sv[tc] = chunk_sum16(ps[0][tc] + ps[1][tc]);
    if constexpr (NW <= 2) {
#pragma unroll
        for (int ph = 0; ph < NW; ph++) {       // wave 0 stores, wave 1 adds (as gram_rhs)
            if (ph > 0) __syncthreads();
            if (wv == ph) {
#pragma unroll
                for (int tc = 0; tc < NTC; tc++)
                    if (kq == 0 && 16 * tc + li < nz) {
                        if constexpr (ULF) g[li] = ul.ge ? sv[0] + ulg : ul.hs ? sv[0] + ul.sc : sv[0];
                        else g[16 * tc + li] = ph ? g[16 * tc + li] + sv[tc] : sv[tc];
                    }
                if (ph == NW - 1 && !ULF) ul_add<NZL, false, true>(R, nullptr, CF, F, nullptr, g, nz, lane, 64);
            }
        }
    } else {
#pragma unroll
        for (int tc = 0; tc < NTC; tc++)
            if (kq == 0) part[wv * NZM + 16 * tc + li] = sv[tc];
        __syncthreads();
        if (tid < nz) {
            double v = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) v += part[w2 * NZM + tid];
            g[tid] = v;
        }
        __syncthreads();
        ul_add<NZL, false, true>(R, nullptr, CF, F, nullptr, g, nz, tid, 64 * NW);
    }
}

// The corrector's right-hand side from slot-owned rows (SRB_RHS_SLOTS; 0 keeps rhs_only everywhere).  Every term row
// with a coefficient belongs to a slot -- VAR, CoM-CoP and obstacle slots their own row, a VEL slot the Z row of its
// variable -- and the slot's lane has just formed that coefficient in a register (set_rhs, polish_stationary).  So
// g = sum_slots cf_slot R[row_slot] needs no CF store, no atomic for the VEL rows and no barrier: each lane adds
// cf * (its slot's row) to NZE private accumulators, and the 64 lanes' partials are summed.  Which instances: one
// wave, one column block of at most 12 columns, stored obstacle rows and the shape compiled in (the conditions of
// the Gram's vector form); every other instance keeps rhs_only.  SRB_RHS_SLOTS_QP 1: the QP stage's copy as well --
// off: with two slot trips and no obstacle rows the sum over the lanes costs more than the shorter pass saves
// (tools/ubench/rhs_bench.hip, profiles/rhs_slots_ubench.txt: the gate passes at the NLP size and fails at the QP size).
#ifndef SRB_RHS_SLOTS
#define SRB_RHS_SLOTS 1
#endif
#ifndef SRB_RHS_SLOTS_QP
#define SRB_RHS_SLOTS_QP 0
#endif
constexpr bool srb_rhs_slots(bool compiled, int NW, int NZL, int NZE)
{
    return SRB_RHS_SLOTS && compiled && NW == 1 && NZL <= 12 && SRB_OBS_STORED(NZL) && NZE > 1 && NZE <= NZL;
}

// g[a] = sum_{t < nts} cfs[t] R[rows[t]][a], a < nz, over the slots of all 64 lanes (one wave).  A slot without a row
// of its own (beyond the last slot, or switched off in the stage) carries cf = 0 and a finite row in range, as in the
// J dx pass.  Rows come through row_load with that pass's two buffers: slot t + 1's row is loaded before slot t's
// FMAs.  The partials are reduced in a fixed order: gram_scatter sums the four 16-lane rows and leaves lane (kq, li)
// with columns kq, kq + 4, kq + 8 at position li, then four DPP butterflies sum the 16 positions; every lane of a
// 16-lane row ends with the same bits, lane li = 0 stores them.  g is left in LDS where rhs_only leaves it.
template <int NZL, int NZE, int TS>
__device__ __forceinline__ void rhs_slots(const double *R, const double (&cfs)[TS], const int (&rows)[TS], int nts, double *g,
                                          int nz, int lane)
{
    static_assert(NZE <= 12 && NZE <= NZL, "rhs_slots: one column block of at most 12 columns");
    constexpr int LDR = NZL + 1;
    const int li = lane & 15, kq = lane >> 4;
    double acc[12];
#pragma unroll
    for (int j = 0; j < 12; j++) acc[j] = 0.0;
    double rw[2][NZE];
    if (0 < nts) row_load<NZE>(R + rows[0] * LDR, rw[0]);
#pragma unroll
    for (int t = 0; t < TS; t++)
        if (t < nts) {
            if (t + 1 < TS && t + 1 < nts) row_load<NZE>(R + rows[(t + 1) % TS] * LDR, rw[(t + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NZE; j++) acc[j] = fma(cfs[t], rw[t & 1][j], acc[j]);
        }
    d4 d = gram_scatter(acc);
#define SRB_RS_STAGE(CTRL) { const double t0_ = dpp_d<CTRL>(d[0]), t1_ = dpp_d<CTRL>(d[1]), t2_ = dpp_d<CTRL>(d[2]); \
                             d[0] += t0_; d[1] += t1_; d[2] += t2_; }
    SRB_RS_STAGE(0xB1) SRB_RS_STAGE(0x4E) SRB_RS_STAGE(0x141) SRB_RS_STAGE(0x140)
#undef SRB_RS_STAGE
    if (li == 0) {
#pragma unroll
        for (int q = 0; q < 3; q++)
            if (kq + 4 * q < nz) g[kq + 4 * q] = d[q];
    }
}
