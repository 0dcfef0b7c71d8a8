// Diagnostic (not product code): cycles per register Gauss-Jordan inverse of an SPD
// NZL x NZL matrix held one row per lane.  Forms: the readlane loop (srb_gj.h gj_invert), an
// interleaved variant of it (gj_interleaved below: the pivot chain issued a link at a time with the
// step's bulk between the links), and the 64-bit DPP row_newbcast broadcast (srb_gj.h
// gj_invert_dpp, rows replicated in each 16-lane row of the wave), each at NZE = NZL and
// NZE = NZL - 1.  Checks that all three give bit-identical inverses.
// Two latency chains go with it: a dependent chain of fp64 FMAs, and a chain of
// FMA -> v_readlane (both halves) -> FMA, in cycles per link.
// The DPP form with the row broadcast folded into the FMA (srb_gj.h gj_invert_dpp_fold, one v_fmac_f64_dpp row_newbcast
// an entry) against the DPP form at (NZL, NZE) = (12, 11), (12, 12), (16, 16), (8, 8), and the reduced solve (srb_solve.h
// la_solve) folded against unfolded at NZE = 11 and 12: five launches each in this one process, fastest and slowest;
// the inverses and the solve results checked bit-equal.  Gate of the folded forms (profiles/dpp_fold_ubench.txt): the
// folded form's slowest launch below the unfolded form's fastest at NZE 11 and at NZE 12.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/gj_bench.hip -o tools/ubench/gj_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#define WAVE 64
#include "../../srb-cbf-nmpc_amd/csrc/srb_kernel_params.h"
#include "../../srb-cbf-nmpc_amd/csrc/srb_gj.h"
#include "../../srb-cbf-nmpc_amd/csrc/srb_solve.h"

// The readlane form with a step's dependent chain -- pivot k's reciprocal (v_rcp_f64 and the two Newton steps of
// rcp_d), the multiplier, the update of entry A[k+1] and its broadcast, pivot k + 1 -- issued one link at a time:
// between two links go the row updates still pending from step k - 1 and step k's broadcasts of the columns just
// updated (bulk(): one column a unit, the update of unit u next to the broadcast of unit u - 1), the order pinned
// by scheduler barriers.  Same operations on the same operands as srb_gj.h gj_invert (checked bit-equal below).
// Measured no faster than gj_invert (profiles/factor_chain_ubench.txt): a dependent fp64 FMA issues at the
// 4-cycle rate with no wait, so spreading the chain hides nothing; the step's cost is its instruction count.
#define SRB_GJ_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int NZL, int NZE = NZL>
__device__ __forceinline__ int gj_interleaved(double (&A)[NZL], int nz, int lane, int regularise)
{
    static_assert(NZE <= NZL && NZE >= 2, "NZE");
    constexpr int UNITS = NZE - 1;                       // a step's units: the columns but its own
    constexpr int GAPS = 9;                             // the gaps of a step's chain the units are dealt over
    int fail = 0;
    double cs = 1.0;
    double rk[NZL];                                   // pivot row k, then (column by column) pivot row k + 1
    double fp = 0.0;                                  // step k - 1's multiplier (its row updates are pending)
    double piv = readlane_d(A[0], 0);
#pragma unroll
    for (int k = 0; k < NZE; k++) {
        // unit u of step k: column (k + 1 + u) % NZE, next pivot row's entry first
        auto upd = [&](int u) {                       // the row update step k - 1 left pending on the column
            const int j = (k + 1 + u) % NZE;
            if (k > 0 && j != k - 1) A[j] = fma(-fp, rk[j], A[j]);
        };
        auto bc = [&](int u) { const int j = (k + 1 + u) % NZE; rk[j] = readlane_d(A[j], k); };
        auto bulk = [&](int g) {                      // gap g: updates of its units, broadcasts of the gap before
            SRB_GJ_FENCE();
#pragma unroll
            for (int u = 0; u < UNITS; u++) {
                if (u * GAPS / UNITS == g) upd(u);
                if (u * GAPS / UNITS == g - 1) bc(u);
            }
            SRB_GJ_FENCE();
        };
        if (regularise && piv <= 1e-14 && piv == piv) piv = 1e-7;
        fail |= !(piv > 0.0);
        double r = __builtin_amdgcn_rcp(piv);         // rcp_d(piv), a link at a time
        bulk(0);
        double e = fma(-piv, r, 1.0);
        bulk(1);
        r = fma(r, e, r);
        bulk(2);
        e = fma(-piv, r, 1.0);
        bulk(3);
        const double inv = fma(r, e, r);
        bulk(4);
        const bool me = lane == k;
        const double fm = A[k] * inv;
        bulk(5);
        const double f = me ? 0.0 : fm;
        bulk(6);
        if (k + 1 < NZE) A[k + 1] = fma(-f, rk[k + 1], A[k + 1]);
        bulk(7);
        if (k + 1 < NZE) piv = readlane_d(A[k + 1], k + 1);
        bulk(8);
        bulk(9);                                      // (the broadcasts of gap 8's units)
        A[k] = me ? 1.0 : -f;
        cs = me ? inv : cs;
        fp = f;
    }
#pragma unroll
    for (int j = 0; j < NZE - 1; j++) A[j] = fma(-fp, rk[j], A[j]);      // the last step's row updates
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] *= cs;
    return fail;
}

// MODE 0 readlane, 1 DPP, 2 interleaved readlane, 3 DPP with the broadcast folded; NZE: the steps run (the matrix is
// NZE x NZE, identity beyond)
template <int NZL, int NZE, int MODE>
__global__ void kern(const double *M, double *out, unsigned long long *cyc, int reps)
{
    const int lane = threadIdx.x;
    const int row = (MODE == 1 || MODE == 3) ? (lane & 15) : lane;
    double A[NZL];
    unsigned long long t0 = 0, t1 = 0;
    for (int rep = 0; rep < reps; rep++) {
#pragma unroll
        for (int j = 0; j < NZL; j++) A[j] = (row < NZE && j < NZE) ? M[row * NZL + j] : (row == j ? 1.0 : 0.0);
        __builtin_amdgcn_sched_barrier(0);
        if (rep == 1) t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MODE == 3) gj_invert_dpp_fold<NZL, NZE>(A, lane, 0);
        else if (MODE == 1) gj_invert_dpp<NZL, NZE>(A, lane, 0);
        else if (MODE == 2) gj_interleaved<NZL, NZE>(A, NZE, lane, 0);
        else gj_invert<NZL, NZE>(A, NZE, lane, 0);
        __builtin_amdgcn_sched_barrier(0);
        double s = 0; for (int j = 0; j < NZL; j++) s += A[j];
        if (s == 12345.678) out[1000] = s;              // keep the work
    }
    __builtin_amdgcn_sched_barrier(0);
    t1 = __builtin_amdgcn_s_memtime();
    if (lane < NZL) for (int j = 0; j < NZL; j++) out[lane * NZL + j] = A[j];
    if (lane == 0) cyc[0] = (t1 - t0) / (reps - 1);
}

// LINKS dependent links, timed as a whole.  RL 0: x = fma(x, a, b);  RL 1: x = fma(readlane(x, 0), a, b), the
// broadcast value an SGPR source of the FMA as in the row updates
template <int RL>
__global__ void chain(const double *M, double *out, unsigned long long *cyc, int reps)
{
    constexpr int LINKS = 64;
    double x = M[threadIdx.x & 7];
    const double a = M[8], b = M[9];
    unsigned long long t0 = 0, t1 = 0;
    for (int rep = 0; rep < reps; rep++) {
        __builtin_amdgcn_sched_barrier(0);
        if (rep == 1) t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < LINKS; i++) x = fma(RL ? readlane_d(x, 0) : x, a, b);
        __builtin_amdgcn_sched_barrier(0);
    }
    t1 = __builtin_amdgcn_s_memtime();
    out[threadIdx.x] = x;
    if (threadIdx.x == 0) cyc[0] = (t1 - t0) / (unsigned long long)((reps - 1) * LINKS);
}

// la_solve (delta = 0, one refinement step) with M the matrix in `Mg` as the "inverse", H and g in LDS; every
// repetition perturbs g by its result, so that no solve can be hoisted out of the loop
template <int NZL, int NZE, bool FOLD>
__global__ void skern(const double *Mg, double *out, unsigned long long *cyc, int reps)
{
    constexpr int LDH = NZL + 1;
    __shared__ double H[16 * LDH], g[16], vy[16], vr[16], vd[16];
    const int lane = threadIdx.x, row = lane & 15;
    for (int e = lane; e < 16 * LDH; e += 64) H[e] = (e / LDH < NZE && e % LDH < NZE) ? Mg[(e / LDH) * NZL + e % LDH] : 0.0;
    if (lane < 16) g[lane] = lane < NZE ? 1.0 / (1 + lane) : 0.0;
    __syncthreads();
    double A[NZL], res[NZL];
#pragma unroll
    for (int j = 0; j < NZL; j++) A[j] = (row < NZE && j < NZE) ? 1e-2 * Mg[row * NZL + j] : 0.0;
    unsigned long long t0 = 0, t1 = 0;
    for (int rep = 0; rep < reps; rep++) {
        __builtin_amdgcn_sched_barrier(0);
        if (rep == 1) t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        la_solve<NZL, 1, NZE, 0, FOLD>(A, H, H, 0.0, g, vy, vr, vd, res, NZE, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (lane < NZE) g[lane] += 1e-3 * res[0];
        __syncthreads();
    }
    __builtin_amdgcn_sched_barrier(0);
    t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) for (int j = 0; j < NZL; j++) out[j] = res[j];
    if (lane == 0) cyc[0] = (t1 - t0) / (reps - 1);
}

// five launches: fastest and slowest; r: the last launch's output
struct MinMax { unsigned long long lo, hi; };
template <class L>
static MinMax launches(L launch, double *dO, unsigned long long *dC, double *r, int nout)
{
    MinMax m{~0ull, 0};
    for (int t = 0; t < 6; t++) {
        launch();
        hipDeviceSynchronize();
        unsigned long long c = 0;
        hipMemcpy(r, dO, nout * sizeof(double), hipMemcpyDeviceToHost);
        hipMemcpy(&c, dC, 8, hipMemcpyDeviceToHost);
        if (t == 0) continue;                         // the first launch loads the code
        m.lo = c < m.lo ? c : m.lo; m.hi = c > m.hi ? c : m.hi;
    }
    return m;
}
// folded against unfolded at one size: the Gauss-Jordan, and (SOLVE) la_solve; returns false on a bit difference;
// gate: set false where the folded form's slowest launch is not below the unfolded form's fastest
template <int NZL, int NZE, bool SOLVE>
static bool fold_ab(const double *dM, double *dO, unsigned long long *dC, bool &gate_gj, bool &gate_solve)
{
    double r0[NZL * NZL], r1[NZL * NZL];
    const MinMax a = launches([&] { hipLaunchKernelGGL((kern<NZL, NZE, 1>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64); }, dO, dC, r0, NZL * NZL);
    const MinMax b = launches([&] { hipLaunchKernelGGL((kern<NZL, NZE, 3>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64); }, dO, dC, r1, NZL * NZL);
    bool eq = !memcmp(r0, r1, sizeof r0);
    gate_gj = b.hi < a.lo;
    printf("NZL=%d NZE=%d GJ: dpp %llu .. %llu cyc, folded %llu .. %llu cyc; folded slowest < dpp fastest: %s; bit-equal: %s\n", NZL, NZE,
           a.lo, a.hi, b.lo, b.hi, gate_gj ? "yes" : "NO", eq ? "yes" : "NO");
    if constexpr (SOLVE) {
        const MinMax c = launches([&] { hipLaunchKernelGGL((skern<NZL, NZE, false>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64); }, dO, dC, r0, NZL);
        const MinMax d = launches([&] { hipLaunchKernelGGL((skern<NZL, NZE, true>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64); }, dO, dC, r1, NZL);
        const bool eqs = !memcmp(r0, r1, NZL * sizeof(double));
        gate_solve = d.hi < c.lo;
        printf("NZL=%d NZE=%d la_solve (with the repetition's LDS update): unfolded %llu .. %llu cyc, folded %llu .. %llu cyc; folded slowest < "
               "unfolded fastest: %s; bit-equal: %s\n", NZL, NZE, c.lo, c.hi, d.lo, d.hi, gate_solve ? "yes" : "NO", eqs ? "yes" : "NO");
        eq = eq && eqs;
    }
    return eq;
}

template <int NZL, int NZE, int MODE>
static unsigned long long run(const double *dM, double *dO, unsigned long long *dC, double *r)
{
    unsigned long long c = 0;
    for (int t = 0; t < 3; t++) {
        hipLaunchKernelGGL((kern<NZL, NZE, MODE>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64);
        hipDeviceSynchronize();
        hipMemcpy(r, dO, NZL * NZL * sizeof(double), hipMemcpyDeviceToHost);
        hipMemcpy(&c, dC, 8, hipMemcpyDeviceToHost);
    }
    return c;
}

int main()
{
    constexpr int NZL = 12;
    double hM[NZL * NZL];
    for (int i = 0; i < NZL; i++)
        for (int j = 0; j < NZL; j++) hM[i * NZL + j] = 1.0 / (1 + i + j) + (i == j ? 2.0 + i : 0.0);
    double *dM, *dO; unsigned long long *dC;
    hipMalloc(&dM, sizeof hM); hipMalloc(&dO, 2048 * sizeof(double)); hipMalloc(&dC, 8);
    hipMemcpy(dM, hM, sizeof hM, hipMemcpyHostToDevice);
    double r[2][3][NZL * NZL];                        // [NZE = NZL, NZL - 1][readlane, dpp, interleaved]
    unsigned long long c[2][3];
    c[0][0] = run<NZL, NZL, 0>(dM, dO, dC, r[0][0]); c[0][1] = run<NZL, NZL, 1>(dM, dO, dC, r[0][1]);
    c[0][2] = run<NZL, NZL, 2>(dM, dO, dC, r[0][2]);
    c[1][0] = run<NZL, NZL - 1, 0>(dM, dO, dC, r[1][0]); c[1][1] = run<NZL, NZL - 1, 1>(dM, dO, dC, r[1][1]);
    c[1][2] = run<NZL, NZL - 1, 2>(dM, dO, dC, r[1][2]);
    // residual of M * inv - I (NZE = NZL)
    double res = 0;
    for (int i = 0; i < NZL; i++) for (int j = 0; j < NZL; j++) { double s = -(i == j); for (int k = 0; k < NZL; k++) s += hM[i * NZL + k] * r[0][0][k * NZL + j]; res = fmax(res, fabs(s)); }
    bool ok = true;
    for (int e = 0; e < 2; e++) {
        const bool eq1 = !memcmp(r[e][0], r[e][1], sizeof r[e][0]), eq2 = !memcmp(r[e][0], r[e][2], sizeof r[e][0]);
        ok = ok && eq1 && eq2;
        printf("NZL=%d NZE=%d readlane GJ %llu cyc, interleaved readlane %llu cyc, dpp GJ %llu cyc; bit-equal to readlane: "
               "interleaved %s, dpp %s\n", NZL, NZL - e, c[e][0], c[e][2], c[e][1], eq2 ? "yes" : "NO", eq1 ? "yes" : "NO");
    }
    printf("|M inv - I| %.3e\n", res);
    // the folded forms (the 12 x 12 matrix above; NZL 16 and 8 take their own)
    bool g11 = false, g12 = false, s11 = false, s12 = false, gx = false, sx = false;
    ok = fold_ab<12, 11, true>(dM, dO, dC, g11, s11) && ok;
    ok = fold_ab<12, 12, true>(dM, dO, dC, g12, s12) && ok;
    {
        double h16[256], h8[64];
        for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++) h16[i * 16 + j] = 1.0 / (1 + i + j) + (i == j ? 2.0 + i : 0.0);
        for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) h8[i * 8 + j] = h16[i * 16 + j];
        double *dM2; hipMalloc(&dM2, sizeof h16);
        hipMemcpy(dM2, h16, sizeof h16, hipMemcpyHostToDevice);
        ok = fold_ab<16, 16, false>(dM2, dO, dC, gx, sx) && ok;
        hipMemcpy(dM2, h8, sizeof h8, hipMemcpyHostToDevice);
        ok = fold_ab<8, 8, false>(dM2, dO, dC, gx, sx) && ok;
    }
    printf("gate (folded slowest < unfolded fastest at NZE 11 and 12): factor %s, solve %s\n", (g11 && g12) ? "passed" : "FAILED",
           (s11 && s12) ? "passed" : "FAILED");
    unsigned long long l0 = 0, l1 = 0;
    const double hc[10] = {0.5, 0.25, 0.125, 0.75, 0.3, 0.6, 0.9, 0.1, 0.5, 0.25};
    hipMemcpy(dM, hc, sizeof hc, hipMemcpyHostToDevice);
    for (int t = 0; t < 3; t++) {
        hipLaunchKernelGGL((chain<0>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64);
        hipDeviceSynchronize(); hipMemcpy(&l0, dC, 8, hipMemcpyDeviceToHost);
        hipLaunchKernelGGL((chain<1>), dim3(1), dim3(64), 0, 0, dM, dO, dC, 64);
        hipDeviceSynchronize(); hipMemcpy(&l1, dC, 8, hipMemcpyDeviceToHost);
    }
    printf("dependent fp64 FMA chain %llu cyc a link; FMA -> v_readlane x2 -> FMA chain %llu cyc a link\n", l0, l1);
    return ok ? 0 : 1;
}
