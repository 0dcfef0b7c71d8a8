// Diagnostic (not product code): cycles per corrector right-hand side g = sum_t CF_t r_t in its two forms (csrc/srb_gram.h,
// the product's text, one wave, NZL = 12, NZE = 11) on LDS data laid out as the solve kernel's at the default shape
// (N = 10, C = 2, K = 11: R with LDR = 13, CF; 64 term rows, 41 U / lambda / slack rows, 112 obstacle rows):
//   rhs_only   lane (kq, li) walks the rows = kq mod 4 of column li, coefficient and element from LDS (CF, R);
//   rhs_slots  every lane adds cf * row for the slots it owns (cf in a register, the row by row_load), then the
//              64 lanes' partials are summed (gram_scatter + four DPP stages).
// Slots as the kernel numbers them: VAR [0, 81) on the Z row of their variable, CoM-CoP [81, 99), VEL [99, 119) on the
// Z row of their velocity, OBS [119, 229) on the obstacle rows.  For rhs_only CF holds, per row, the sum of its slots'
// coefficients (the VAR slot's store, then the VEL slot's atomic add).  Three sizes:
//   qp2   nko = 0, two slot trips   (the QP stage as the kernel runs it: ceil((n + 2 (N - 1)) / 64) = 2);
//   qp3   nko = 0, three slot trips (the third trip's slots carry cf = 0);
//   nlp   all four trips, the 110 obstacle rows.
// The slots that are off at a size (VEL and OBS in the QP stage) carry cf = 0, as in the kernel.
// s_memtime cycles: every launch times 32 repetitions (after a warm-up) and reports their median; five launches a form
// and size.  Gate: the new form's slowest launch below the old form's fastest.  Both g against a long-double sum on the
// host from the same R and coefficients, in units of 2^-52 sum |cf r_a| (an ulp of the sum of magnitudes: each of the at
// most 48 + 6 roundings of a lane's chain and the reduction is below half an ulp of a partial sum, itself below that
// sum; random signs keep the total to a few): at most 4.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 tools/ubench/rhs_bench.hip -o tools/ubench/rhs_bench
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define WAVE 64
#include "../../srb-cbf-nmpc_amd/csrc/srb_gram.h"

constexpr int NZL = 12, NZE = 11, LDR = NZL + 1;
constexpr int N = 10, C = 2, K = 11, NV = (6 + C) * N + 1;             // n = 81
constexpr int RU = 64, RO = 112, NKP = 112, TT = RO + NKP;             // the kernel's rU, rO, NKP, TT at this shape, NW = 1
constexpr int TS = 4, NE = 2 * (N - 1), SE = NV, SV = SE + NE, SO = SV + 2 * N, S = SO + N * K;
constexpr int REPS = 33;                                               // the first is the warm-up
constexpr int LAUNCHES = 5;

template <bool SLOTS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) kern(const double *Rg, const double *CFg, const double *cfg, const int *rowg, int nko, int nts, double *out, unsigned long long *cyc)
{
    __shared__ double R[TT * LDR], CF[TT + 1], g[16];
    const int tid = threadIdx.x;
    for (int e = tid; e < TT * LDR; e += 64) R[e] = Rg[e];
    for (int e = tid; e <= TT; e += 64) CF[e] = CFg[e];
    if (tid < 16) g[tid] = -1.0;
    ObsFold F;
    F.OJ = nullptr; F.FO = nullptr; F.rO = RO; F.N = N; F.K = K; F.NOP = 0; F.mask = 0; F.rU = RU; F.C = C; F.n = NV;
    double cfs[TS];
    int rows[TS];
#pragma unroll
    for (int t = 0; t < TS; t++) { cfs[t] = cfg[tid + 64 * t]; rows[t] = rowg[tid + 64 * t]; }
    srb_sync<1>();
    for (int rep = 0; rep < REPS; rep++) {
        // nothing of a repetition is carried over from the one before: the coefficients and rows are opaque again
#pragma unroll
        for (int t = 0; t < TS; t++) asm volatile("" : "+v"(cfs[t]), "+v"(rows[t]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SLOTS) rhs_slots<NZL, NZE, TS>(R, cfs, rows, nts, g, NZE, tid);
        else rhs_only<NZL, 1>(R, CF, RU, F, nko, g, NZE, tid, nullptr, ~0ull);
        srb_sync<1>();
        const double keep = g[tid & 15];                               // the stores have landed before the stamp
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if (keep == 12345.678) out[1000] = keep;
        if (tid == 0) cyc[rep] = t1 - t0;
    }
    if (tid < 16) out[tid] = g[tid];
}

struct Data { std::vector<double> R, CF, cf; std::vector<int> row; };

// term row of slot s (the kernel's slot_init), -1 beyond the last slot
static int slot_row(int s)
{
    if (s < SE) return s < 4 * N ? s : s + (RU - 4 * N);
    if (s < SV) return 4 * N + (s - SE);
    if (s < SO) { const int tt = s - SV; return 4 * (tt % N) + (tt < N ? 1 : 3); }
    if (s < S) return RO + (s - SO);
    return -1;
}

// R as the kernel's rows are filled (uniform in (-1, 1)); the slots' coefficients of the stage (uniform in (-1, 1); 0 for
// the slots the stage switches off and beyond the last slot, which read row 0); CF their per-row sums
static Data make(bool nlp, unsigned seed)
{
    Data d;
    d.R.assign(TT * LDR, 0.0); d.CF.assign(TT + 1, 0.0); d.cf.assign(64 * TS, 0.0); d.row.assign(64 * TS, 0);
    srand(seed);
    auto val = [&]() { return 2.0 * rand() / RAND_MAX - 1.0; };
    auto row = [&](int r, int c0, int c1) { for (int c = c0; c < c1; c++) d.R[r * LDR + c] = val(); };
    for (int r = 0; r < 4 * N; r++) row(r, 0, (r / 4 + 1) * (C - 1) + 1);
    for (int e = 0; e < NE; e++) row(4 * N + e, 0, (e / 2 + 2) * (C - 1) + 1);
    for (int j = 0; j < N; j++) {
        for (int u = 0; u < 2; u++) row(RU + 2 * j + u, 1 + j, 2 + j);
        for (int u = 0; u < C; u++) row(RU + 2 * N + C * j + u, 1 + j, 2 + j);
    }
    d.R[(RU + NV - 1 - 4 * N) * LDR] = 1.0;                                              // the slack row, Z = e_0
    for (int o = 0; o < N * K; o++) row(RO + o, 0, (o / K + 1) * (C - 1) + 1);
    for (int s = 0; s < 64 * TS; s++) {
        const int r = slot_row(s);
        d.row[s] = r < 0 ? 0 : r;
        d.cf[s] = (r < 0 || (!nlp && s >= SV)) ? 0.0 : val();
    }
    for (int s = 0; s < S; s++) d.CF[d.row[s]] += d.cf[s];                             // slot order: the store, then the VEL add
    return d;
}

static double *dR, *dCF, *dcf, *dO;
static int *drow;
static unsigned long long *dC;

template <bool SLOTS>
static bool run(const char *name, const char *size, const Data &d, int nko, int nts, unsigned long long *fast, unsigned long long *slow)
{
    (void)hipMemcpy(dR, d.R.data(), d.R.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dCF, d.CF.data(), d.CF.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dcf, d.cf.data(), d.cf.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(drow, d.row.data(), d.row.size() * 4, hipMemcpyHostToDevice);
    double o[16];
    unsigned long long med[LAUNCHES], lo = ~0ull, hi = 0;
    for (int l = 0; l < LAUNCHES; l++) {
        unsigned long long c[REPS];
        hipLaunchKernelGGL((kern<SLOTS>), dim3(1), dim3(64), 0, 0, dR, dCF, dcf, drow, nko, nts, dO, dC);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(2); }
        (void)hipMemcpy(c, dC, sizeof c, hipMemcpyDeviceToHost);
        std::sort(c + 1, c + REPS);
        med[l] = c[1 + (REPS - 1) / 2];
        lo = std::min(lo, c[1]); hi = std::max(hi, c[REPS - 1]);
    }
    (void)hipMemcpy(o, dO, sizeof o, hipMemcpyDeviceToHost);
    // the host's sum over the slots the call covers (rhs_only covers the same through CF: a slot beyond nts has cf = 0)
    double worst = 0.0;
    for (int a = 0; a < NZE; a++) {
        long double ref = 0.0L, mag = 0.0L;
        for (int s = 0; s < 64 * nts; s++) {
            const long double p = (long double)d.cf[s] * (long double)d.R[d.row[s] * LDR + a];
            ref += p; mag += fabsl(p);
        }
        const double err = (double)fabsl((long double)o[a] - ref), ulp = 0x1p-52 * (double)mag;
        worst = std::max(worst, ulp > 0.0 ? err / ulp : (err == 0.0 ? 0.0 : INFINITY));
    }
    const bool ok = worst <= 4.0;
    *fast = *std::min_element(med, med + LAUNCHES); *slow = *std::max_element(med, med + LAUNCHES);
    printf("%-9s %-3s launch medians %5llu %5llu %5llu %5llu %5llu  (any repetition: min %5llu max %5llu)   g against the host: %s (largest error %.3f ulp of sum |terms|)\n",
           name, size, med[0], med[1], med[2], med[3], med[4], lo, hi, ok ? "ok" : "FAIL", worst);
    return ok;
}

int main()
{
    (void)hipMalloc(&dR, TT * LDR * 8); (void)hipMalloc(&dCF, (TT + 1) * 8); (void)hipMalloc(&dcf, 64 * TS * 8);
    (void)hipMalloc(&drow, 64 * TS * 4); (void)hipMalloc(&dO, 2048 * 8); (void)hipMalloc(&dC, REPS * 8);
    bool ok = true;
    const struct { const char *name; bool nlp; int nko, nts; } sz[3] = {{"qp2", false, 0, 2}, {"qp3", false, 0, 3}, {"nlp", true, NKP, 4}};
    for (int i = 0; i < 3; i++) {
        const Data d = make(sz[i].nlp, 11 + i);
        unsigned long long of, os, nf, ns;
        ok &= run<false>("rhs_only", sz[i].name, d, sz[i].nko, sz[i].nts, &of, &os);
        ok &= run<true>("rhs_slots", sz[i].name, d, sz[i].nko, sz[i].nts, &nf, &ns);
        printf("gate %s: rhs_slots' slowest launch %llu below rhs_only's fastest %llu: %s\n", sz[i].name, ns, of, ns < of ? "yes" : "no");
    }
    return ok ? 0 : 1;
}
