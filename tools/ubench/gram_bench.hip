// Diagnostic (not product code): cycles per reduced Gram + right-hand side (csrc/srb_gram.h gram_rhs and gram_rhs_vec, the product's
// text, one wave, NZL = 12, NZE = 11) on LDS data laid out as the solve kernel's at the default shape (N = 10, C = 2,
// K = 11: R with LDR = 13, W, CF; 64 term rows, 41 U / lambda / slack rows, 112 obstacle rows), at 16 term groups
// (the QP Gram) and at 44 (the NLP Gram: + 7 obstacle batches).  Three forms of the accumulation:
//   (a) SRB_GRAM_MFMA     v_mfma_f64_16x16x4_f64 on one accumulator tile;
//   (b) SRB_GRAM_DPP_ASM  one column of H per lane, v_fmac_f64_dpp row_newbcast (inline assembly), the batches
//                         unrolled and the accumulators above a group's highest non-zero column left out;
//   (c) SRB_GRAM_DPP_MOV  the same with bc16() + fma(): v_mov_b64_dpp + v_fmac_f64, no assembly.
// s_memtime cycles of every repetition of one launch: min / median / max.  H and g of each form against a host
// computation: exact for small-integer operands, within (number of terms) 2^-52 sum |w r_a r_b| (g: sum |cf r_a|)
// for random ones.  Two chains go with it: dependent and independent v_fmac_f64_dpp, and the same of plain
// v_fmac_f64, in cycles an instruction.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 tools/ubench/gram_bench.hip -o tools/ubench/gram_bench
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define WAVE 64
#include "../../srb-cbf-nmpc_amd/csrc/srb_gram.h"

constexpr int NZL = 12, NZE = 11, LDR = NZL + 1, LDH = NZL + 1;
constexpr int N = 10, C = 2, K = 11, NV = (6 + C) * N + 1;             // n = 81
constexpr int RU = 64, RO = 112, NKP = 112, TT = RO + NKP;             // the kernel's rU, rO, NKP, TT at this shape, NW = 1
constexpr int REPS = 33;                                               // the first is the warm-up

template <int FORM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) kern(const double *Rg, const double *Wg, const double *CFg, int nko, double *out, unsigned long long *cyc)
{
    __shared__ double R[TT * LDR], W[TT], CF[TT], H[NZL * LDH], g[16];
    const int tid = threadIdx.x;
    for (int e = tid; e < TT * LDR; e += 64) R[e] = Rg[e];
    for (int e = tid; e < TT; e += 64) { W[e] = Wg[e]; CF[e] = CFg[e]; }
    for (int e = tid; e < NZL * LDH; e += 64) H[e] = -1.0;
    if (tid < 16) g[tid] = -1.0;
    ObsFold F;
    F.OJ = nullptr; F.FO = nullptr; F.rO = RO; F.N = N; F.K = K; F.NOP = 0; F.mask = 0; F.rU = RU; F.C = C; F.n = NV;
    srb_sync<1>();
    for (int rep = 0; rep < REPS; rep++) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (FORM == SRB_GRAM_MFMA) gram_rhs<NZL, true, 1>(R, W, CF, RU, F, nko, H, g, NZE, tid, nullptr, ~0ull);
        else gram_rhs_vec<NZL, true, GramShape<N, C, K>, FORM>(R, W, CF, F, nko, H, g, NZE, tid);
        srb_sync<1>();
        const double keep = H[tid % (NZL * LDH)] + g[tid & 15];        // the stores have landed before the stamp
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if (keep == 12345.678) out[1000] = keep;
        if (tid == 0) cyc[rep] = t1 - t0;
    }
    for (int e = tid; e < NZL * LDH; e += 64) out[e] = H[e];
    if (tid < 16) out[NZL * LDH + tid] = g[tid];
}

// LINKS instructions timed as a whole.  DPP 1: v_fmac_f64_dpp row_newbcast (the broadcast operand loop-invariant), 0: plain
// v_fmac_f64.  IND 0: one accumulator (a dependent chain), 1: eight accumulators in turn.
#define GB_F8(OP, SFX) OP " %0, %8, %9" SFX "\n\t" OP " %1, %8, %9" SFX "\n\t" OP " %2, %8, %9" SFX "\n\t" OP " %3, %8, %9" SFX "\n\t" \
                       OP " %4, %8, %9" SFX "\n\t" OP " %5, %8, %9" SFX "\n\t" OP " %6, %8, %9" SFX "\n\t" OP " %7, %8, %9" SFX "\n\t"
#define GB_D8(OP, SFX) OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t" \
                       OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t" OP " %0, %8, %9" SFX "\n\t"
#define GB_DPP " row_newbcast:3 row_mask:0xf bank_mask:0xf"
template <int DPP, int IND>
__global__ void chain(const double *M, double *out, unsigned long long *cyc, int reps)
{
    constexpr int LINKS = 64;
    double x[8];
    for (int i = 0; i < 8; i++) x[i] = M[(threadIdx.x + i) & 7];
    const double a = M[8] * (1 + (threadIdx.x & 15)), b = M[9];
    unsigned long long t0 = 0, t1 = 0;
    for (int rep = 0; rep < reps; rep++) {
        __builtin_amdgcn_sched_barrier(0);
        if (rep == 1) t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 1" : : "v"(a));           // a is loop-invariant: its one write is two wait states behind here
#pragma unroll
        for (int i = 0; i < LINKS / 8; i++) {
#define GB_STMT(S) asm volatile(S :"+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]) : "v"(a), "v"(b))
            if (DPP && IND) GB_STMT(GB_F8("v_fmac_f64_dpp", GB_DPP));
            else if (DPP) GB_STMT(GB_D8("v_fmac_f64_dpp", GB_DPP));
            else if (IND) GB_STMT(GB_F8("v_fmac_f64", ""));
            else GB_STMT(GB_D8("v_fmac_f64", ""));
#undef GB_STMT
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    t1 = __builtin_amdgcn_s_memtime();
    double s = 0.0;
    for (int i = 0; i < 8; i++) s += x[i];
    out[threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[0] = (t1 - t0) * 100 / (unsigned long long)((reps - 1) * LINKS);     // hundredths of a cycle
}

struct Data { std::vector<double> R, W, CF; };

// small: integers (every product and sum exact); else uniform in (-1, 1), weights in (0, 1)
static Data make(bool small, unsigned seed)
{
    Data d;
    d.R.assign(TT * LDR, 0.0); d.W.assign(TT, 0.0); d.CF.assign(TT, 0.0);
    srand(seed);
    auto val = [&]() { return small ? (double)(rand() % 5 - 2) : 2.0 * rand() / RAND_MAX - 1.0; };
    auto wgt = [&]() { return small ? (double)(rand() % 4) : (double)rand() / RAND_MAX; };
    auto row = [&](int r, int c0, int c1) { for (int c = c0; c < c1; c++) d.R[r * LDR + c] = val(); d.W[r] = wgt(); d.CF[r] = val(); };
    // state rows of grid k and CoM-CoP rows of grid i: non-zero up to the columns of grid k and i + 1 (the rest of [0, RU) padding)
    for (int r = 0; r < 4 * N; r++) row(r, 0, (r / 4 + 1) * (C - 1) + 1);
    for (int e = 0; e < 2 * (N - 1); e++) row(4 * N + e, 0, (e / 2 + 2) * (C - 1) + 1);
    for (int j = 0; j < N; j++) {                                                       // U and lambda rows: their grid's column
        for (int u = 0; u < 2; u++) row(RU + 2 * j + u, 1 + j, 2 + j);
        for (int u = 0; u < C; u++) row(RU + 2 * N + C * j + u, 1 + j, 2 + j);
    }
    const int rs = RU + NV - 1 - 4 * N;
    row(rs, 0, 1); d.R[rs * LDR] = 1.0;                                                 // the slack row, Z = e_0
    for (int o = 0; o < N * K; o++) row(RO + o, 0, (o / K + 1) * (C - 1) + 1);          // obstacle rows (110 of 112): their grid's state rows
    return d;
}

// H, g and the bounds' sums on the host over the rows the call covers
static void host(const Data &d, int nko, double *H, double *g, double *Ha, double *ga, int &terms)
{
    for (int e = 0; e < NZL * NZL; e++) H[e] = Ha[e] = 0.0;
    for (int e = 0; e < NZL; e++) g[e] = ga[e] = 0.0;
    terms = 0;
    for (int r = 0; r < RO + nko; r++) {
        if (r >= RU + NV - 4 * N && r < RO) continue;
        terms++;
        for (int a = 0; a < NZL; a++) {
            g[a] += d.CF[r] * d.R[r * LDR + a]; ga[a] += fabs(d.CF[r] * d.R[r * LDR + a]);
            for (int b = 0; b < NZL; b++) {
                const double p = d.W[r] * d.R[r * LDR + a] * d.R[r * LDR + b];
                H[a * NZL + b] += p; Ha[a * NZL + b] += fabs(p);
            }
        }
    }
}

static double *dR, *dW, *dCF, *dO;
static unsigned long long *dC;

template <int FORM>
static bool run(const char *name, const Data &d, bool small, int nko, unsigned long long *mn, unsigned long long *mx)
{
    (void)hipMemcpy(dR, d.R.data(), d.R.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dW, d.W.data(), TT * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dCF, d.CF.data(), TT * 8, hipMemcpyHostToDevice);
    double o[NZL * LDH + 16];
    unsigned long long c[REPS];
    for (int t = 0; t < 2; t++) {
        hipLaunchKernelGGL((kern<FORM>), dim3(1), dim3(64), 0, 0, dR, dW, dCF, nko, dO, dC);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(2); }
    }
    (void)hipMemcpy(o, dO, sizeof o, hipMemcpyDeviceToHost);
    (void)hipMemcpy(c, dC, sizeof c, hipMemcpyDeviceToHost);
    std::sort(c + 1, c + REPS);
    double H[NZL * NZL], g[NZL], Ha[NZL * NZL], ga[NZL];
    int terms;
    host(d, nko, H, g, Ha, ga, terms);
    double worst = 0.0;                                   // largest error in units of its bound (exact data: any error is inf)
    for (int a = 0; a < NZL; a++) {
        for (int b = 0; b <= NZL; b++) {
            const bool isg = b == NZL;
            if (isg && a >= NZE) continue;                // g holds nz entries
            const double got = isg ? o[NZL * LDH + a] : o[a * LDH + b], ref = isg ? g[a] : H[a * NZL + b];
            const double bound = small ? 0.0 : terms * 0x1p-52 * (isg ? ga[a] : Ha[a * NZL + b]);
            const double err = fabs(got - ref);
            if (!(err <= bound)) worst = (bound > 0.0) ? fmax(worst, err / bound) : INFINITY;
            else if (bound > 0.0) worst = fmax(worst, err / bound);
        }
    }
    const bool ok = worst <= 1.0;
    printf("%-8s %2d groups %-7s cycles min %5llu median %5llu max %5llu   H, g against the host: %s (worst error / bound %.3f)\n",
           name, (RU + nko) / 4, small ? "integer" : "random", c[1], c[1 + (REPS - 1) / 2], c[REPS - 1], ok ? "ok" : "FAIL", worst);
    *mn = c[1]; *mx = c[REPS - 1];
    return ok;
}

template <int DPP, int IND>
static double run_chain()
{
    unsigned long long c = 0;
    for (int t = 0; t < 3; t++) {
        hipLaunchKernelGGL((chain<DPP, IND>), dim3(1), dim3(64), 0, 0, dR, dO, dC, 64);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(&c, dC, 8, hipMemcpyDeviceToHost);
    }
    return c / 100.0;
}

int main()
{
    (void)hipMalloc(&dR, TT * LDR * 8); (void)hipMalloc(&dW, TT * 8); (void)hipMalloc(&dCF, TT * 8); (void)hipMalloc(&dO, 2048 * 8); (void)hipMalloc(&dC, REPS * 8);
    bool ok = true;
    unsigned long long mn[3][2], mx[3][2];
    for (int small = 1; small >= 0; small--) {
        const Data d = make(small, 7 + small);
        for (int s = 0; s < 2; s++) {
            const int nko = s ? NKP : 0;
            ok &= run<SRB_GRAM_MFMA>("mfma", d, small, nko, &mn[0][s], &mx[0][s]);
            ok &= run<SRB_GRAM_DPP_ASM>("dpp-asm", d, small, nko, &mn[1][s], &mx[1][s]);
            ok &= run<SRB_GRAM_DPP_MOV>("dpp-mov", d, small, nko, &mn[2][s], &mx[2][s]);
        }
    }
    // the gate for building a vector form, on the random data's timings: a vector form's slowest below the MFMA form's fastest at both sizes
    for (int f = 1; f < 3; f++)
        printf("%s: slowest below the mfma form's fastest at 16 groups %s, at 44 groups %s\n", f == 1 ? "dpp-asm" : "dpp-mov",
               mx[f][0] < mn[0][0] ? "yes" : "no", mx[f][1] < mn[0][1] ? "yes" : "no");
    const double hc[10] = {0.5, 0.25, 0.125, 0.75, 0.3, 0.6, 0.9, 0.1, 1e-3, 0.25};
    (void)hipMemcpy(dR, hc, sizeof hc, hipMemcpyHostToDevice);
    printf("v_fmac_f64_dpp row_newbcast: dependent %.2f cycles an instruction, independent (8 accumulators) %.2f\n",
           run_chain<1, 0>(), run_chain<1, 1>());
    printf("v_fmac_f64:                  dependent %.2f cycles an instruction, independent (8 accumulators) %.2f\n",
           run_chain<0, 0>(), run_chain<0, 1>());
    return ok ? 0 : 1;
}
