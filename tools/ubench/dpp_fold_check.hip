// Diagnostic (not product code): the DPP Gauss-Jordan and the DPP reduced solve of the solve kernel with the row
// broadcast folded into the FMA (csrc/srb_gj.h gj_invert_dpp_fold, csrc/srb_solve.h la_solve<.., FOLD = true>) against
// the bc16() + fma() text (gj_invert_dpp, la_solve<.., FOLD = false>), both compiled from the product headers into
// this one binary and compared bit for bit: the inverse of every lane, the failure flag and the solve result.
// Sizes (NZL, NZE, nz) = (8, 8, 3), (12, 12, 4), (12, 11, 11), (12, 12, 12), (16, 16, 16).  Matrices: a well-conditioned
// SPD matrix; an SPD matrix with diagonal weights up to 1e12 (the barrier's range); a matrix with a pivot <= 1e-14 with
// `regularise` on and off; an indefinite matrix; a matrix with one NaN entry (flags and NaN pattern equal; the NaNs'
// own sign and payload bits follow the FMA's operand order and are not compared).  Each with delta = 0 and delta != 0 (the
// shift applied by gj_load and, on the fly, by la_solve), the solve with the compile-time refinement count and with
// the run-time one of the fp32-factor instances (KF, three steps).  Prints one line a size and the number of
// mismatching cases; exit status 0 only if there is none.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/dpp_fold_check.hip -o dpp_fold_check
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <cstdlib>
#define HIP(x) do { if ((x) != hipSuccess) { printf("%s failed\n", #x); exit(2); } } while (0)
#define WAVE 64
#include "../../srb-cbf-nmpc_amd/csrc/srb_kernel_params.h"
#include "../../srb-cbf-nmpc_amd/csrc/srb_solve.h"

#if !SRB_USE_DPP
#error "the folded forms exist only under SRB_USE_DPP"
#endif

// out: [form 0 unfolded, 1 folded][64 lanes][3 NZL: inverse | solve | KF solve], flag: [form]
template <int NZL, int NZE>
__global__ void check(const double *Hg, const double *Zg, const double *gg, double delta, int nz, int regularise, double *out,
                      int *flag)
{
    constexpr int LDH = NZL + 1;
    // 16 rows: la_solve's lanes >= NZL of a 16-lane row read (and discard) rows beyond the matrix
    __shared__ double H[16 * LDH], ZZ[16 * LDH], g[16], vy[16], vr[16], vd[16];
    const int lane = threadIdx.x;
    for (int e = lane; e < 16 * LDH; e += 64) {
        const int i = e / LDH, j = e % LDH;
        const bool in = i < nz && j < nz;
        H[e] = in ? Hg[i * nz + j] : 0.0;
        ZZ[e] = in ? Zg[i * nz + j] : 0.0;
    }
    if (lane < 16) g[lane] = lane < nz ? gg[lane] : 0.0;
    __syncthreads();
    double A0[NZL], A1[NZL];
    gj_load<NZL, NZE>(A0, H, ZZ, delta, nz, lane);
    gj_load<NZL, NZE>(A1, H, ZZ, delta, nz, lane);
    const int f0 = gj_invert_dpp<NZL, NZE>(A0, lane, regularise);
    const int f1 = gj_invert_dpp_fold<NZL, NZE>(A1, lane, regularise);
    if (lane == 0) { flag[0] = f0; flag[1] = f1; }
    double *o0 = out + lane * 3 * NZL, *o1 = out + (64 + lane) * 3 * NZL;
#pragma unroll
    for (int j = 0; j < NZL; j++) { o0[j] = A0[j]; o1[j] = A1[j]; }
    // the solves take one inverse, the unfolded one, so that a difference is the solve's own
    double r0[NZL], r1[NZL];
    la_solve<NZL, 1, NZE, 0, false>(A0, H, ZZ, delta, g, vy, vr, vd, r0, nz, lane);
    la_solve<NZL, 1, NZE, 0, true>(A0, H, ZZ, delta, g, vy, vr, vd, r1, nz, lane);
#pragma unroll
    for (int j = 0; j < NZL; j++) { o0[NZL + j] = r0[j]; o1[NZL + j] = r1[j]; }
    la_solve<NZL, 1, NZE, 1, false>(A0, H, ZZ, delta, g, vy, vr, vd, r0, nz, lane, 3);
    la_solve<NZL, 1, NZE, 1, true>(A0, H, ZZ, delta, g, vy, vr, vd, r1, nz, lane, 3);
#pragma unroll
    for (int j = 0; j < NZL; j++) { o0[2 * NZL + j] = r0[j]; o1[2 * NZL + j] = r1[j]; }
}

static unsigned long long rng = 0x9E3779B97F4A7C15ull;
static double urand()
{
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng >> 11) / 9007199254740992.0;
}

// B B' + d I over nz x nz
static std::vector<double> spd(int nz, double d)
{
    std::vector<double> B(nz * nz), M(nz * nz);
    for (auto &v : B) v = 2.0 * urand() - 1.0;
    for (int i = 0; i < nz; i++)
        for (int j = 0; j < nz; j++) {
            double s = (i == j) ? d : 0.0;
            for (int k = 0; k < nz; k++) s += B[i * nz + k] * B[j * nz + k];
            M[i * nz + j] = s;
        }
    return M;
}

// the words differ: in their bits, or (nan_pattern) in their bits with at most one of them a NaN
static int differs(double a, double b, bool nan_pattern)
{
    if (nan_pattern && std::isnan(a) && std::isnan(b)) return 0;
    return memcmp(&a, &b, 8) != 0;
}

enum { SPD, WIDE, TINY_REG, TINY_NOREG, INDEF, ONE_NAN, NKIND };
static const char *KIND[NKIND] = {"spd", "weights-1e12", "tiny-pivot-reg", "tiny-pivot-noreg", "indefinite", "one-nan"};

template <int NZL, int NZE>
static int run_size(int nz, double *dH, double *dZ, double *dg, double *dO, int *dF)
{
    int bad = 0, nfail = 0, nnan = 0;
    std::vector<double> o(2 * 64 * 3 * NZL);
    for (int kind = 0; kind < NKIND; kind++)
        for (int sh = 0; sh < 2; sh++) {
            std::vector<double> H = spd(nz, (double)nz), Z = spd(nz, 1.0), g(16, 0.0);
            for (int i = 0; i < nz; i++) g[i] = 2.0 * urand() - 1.0;
            if (kind == WIDE) for (int i = 0; i < nz; i++) H[i * nz + i] += pow(10.0, 12.0 * (i + 1) / nz);
            if (kind == TINY_REG || kind == TINY_NOREG) {
                for (int j = 0; j < nz; j++) H[j] = H[j * nz] = 0.0;      // first pivot alone in its row and column
                H[0] = 1e-15;
            }
            if (kind == INDEF) H[1 * nz + 1] = -1.0;
            if (kind == ONE_NAN) H[1 * nz + 2] = NAN;
            const double delta = sh ? 1e-3 : 0.0;
            const int reg = (kind == TINY_NOREG || kind == INDEF) ? 0 : 1;
            HIP(hipMemcpy(dH, H.data(), nz * nz * sizeof(double), hipMemcpyHostToDevice));
            HIP(hipMemcpy(dZ, Z.data(), nz * nz * sizeof(double), hipMemcpyHostToDevice));
            HIP(hipMemcpy(dg, g.data(), 16 * sizeof(double), hipMemcpyHostToDevice));
            HIP(hipMemset(dO, 0xff, o.size() * sizeof(double)));
            hipLaunchKernelGGL((check<NZL, NZE>), dim3(1), dim3(64), 0, 0, dH, dZ, dg, delta, nz, reg, dO, dF);
            if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1000; }
            int f[2];
            HIP(hipMemcpy(o.data(), dO, o.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(f, dF, sizeof f, hipMemcpyDeviceToHost));
            // the NaN matrix: flags and NaN pattern equal (a NaN where the other form has one, every other word
            // bit-equal) -- which of an FMA's NaN operands lends its sign and payload depends on the operand order, and
            // the DPP operand has to be the first; every other matrix: memcmp
            bool eq = f[0] == f[1];
            if (kind == ONE_NAN) {
                for (int e = 0; e < 64 * 3 * NZL; e++) eq = eq && differs(o[e], o[64 * 3 * NZL + e], true) == 0;
            } else {
                eq = eq && !memcmp(o.data(), o.data() + 64 * 3 * NZL, 64 * 3 * NZL * sizeof(double));
            }
            nfail += f[0];
            for (int e = 0; e < NZL; e++) nnan += std::isnan(o[e]);
            if (!eq) {
                bad++;
                int inv = 0, sol = 0, kf = 0;
                for (int l = 0; l < 64; l++)
                    for (int j = 0; j < 3 * NZL; j++)
                        if (differs(o[l * 3 * NZL + j], o[(64 + l) * 3 * NZL + j], kind == ONE_NAN)) (j < NZL ? inv : j < 2 * NZL ? sol : kf)++;
                printf("  MISMATCH NZL=%d NZE=%d nz=%d %s delta=%g: flags %d / %d, differing words: inverse %d, solve %d, KF solve %d\n",
                       NZL, NZE, nz, KIND[kind], delta, f[0], f[1], inv, sol, kf);
            }
        }
    printf("NZL=%d NZE=%d nz=%d: %d cases, %d flagged not PD, %d NaN words in lane 0's inverse rows, %d mismatches\n", NZL, NZE, nz,
           2 * NKIND, nfail, nnan, bad);
    return bad;
}

int main()
{
    double *dH, *dZ, *dg, *dO; int *dF;
    HIP(hipMalloc(&dH, 256 * sizeof(double))); HIP(hipMalloc(&dZ, 256 * sizeof(double))); HIP(hipMalloc(&dg, 16 * sizeof(double)));
    HIP(hipMalloc(&dO, 2 * 64 * 3 * 16 * sizeof(double))); HIP(hipMalloc(&dF, 2 * sizeof(int)));
    int bad = 0;
    bad += run_size<8, 8>(3, dH, dZ, dg, dO, dF);
    bad += run_size<12, 12>(4, dH, dZ, dg, dO, dF);
    bad += run_size<12, 11>(11, dH, dZ, dg, dO, dF);
    bad += run_size<12, 12>(12, dH, dZ, dg, dO, dF);
    bad += run_size<16, 16>(16, dH, dZ, dg, dO, dF);
    printf("mismatches: %d\n", bad);
    return bad ? 1 : 0;
}
