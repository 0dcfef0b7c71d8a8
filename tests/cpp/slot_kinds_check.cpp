// Stand-alone check of the per-trip slot-kind tables of srb_kernel_params.h against the run-time rule
// (tests/test_slot_kinds.py builds and runs it; no GPU).  Exit status 0 when every check holds.
#include <cstdio>

#include "srb_kernel_params.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the kind of slot sl as slot_init decides it, written out here on its own
static int kind_by_ranges(int sl, int N, int C, int K)
{
    const int n = (6 + C) * N + 1, sE = n, sV = sE + 2 * (N - 1), sO = sV + 2 * N, S = sO + N * K;
    if (sl < sE) return SRB_K_VAR;
    if (sl < sV) return SRB_K_COP;
    if (sl < sO) return SRB_K_VEL;
    if (sl < S) return SRB_K_OBS;
    return SRB_K_NONE;
}

// one compiled-shape instance (NZL, TS, NW, NC, CC, KC of SRB_KERNEL_INSTANCES)
static void compiled(int TS, int NW, int N, int C, int K)
{
    const int NTH = 64 * NW, n = (6 + C) * N + 1, sE = n, sV = sE + 2 * (N - 1), sO = sV + 2 * N, S = sO + N * K;
    CHECK(srb_slots(N, C, K) == S, "shape %d %d %d", N, C, K);
    CHECK(S <= NTH * TS, "shape %d %d %d: %d slots, %d lanes x trips", N, C, K, S, NTH * TS);
    CHECK(srb_trips_cover(N, C, K, NTH, TS), "shape %d %d %d", N, C, K);
    for (int t = 0; t < TS; t++) {
        const int km = srb_trip_kinds(N, C, K, NTH, t), rows = srb_trip_rows(N, C, K, NTH, t);
        bool all_single = true, all_on = true, any_com = false;
        int seen = 0;
        for (int tid = 0; tid < NTH; tid++) {
            const int sl = tid + NTH * t, kd = kind_by_ranges(sl, N, C, K);
            CHECK(srb_slot_kind(sl, sE, sV, sO, S) == kd, "slot %d", sl);
            CHECK(km & SRB_KM(kd), "shape %d %d %d trip %d tid %d: kind %d not in mask 0x%x", N, C, K, t, tid, kd, km);
            seen |= SRB_KM(kd);
            all_single = all_single && (kd == SRB_K_OBS || kd == SRB_K_NONE);
            all_on = all_on && kd == SRB_K_VAR && sl < n - 1;
            any_com = any_com || sl < 4 * N;
        }
        CHECK(seen == km, "shape %d %d %d trip %d: mask 0x%x, kinds seen 0x%x", N, C, K, t, km, seen);   // and no wider
        CHECK((rows == 1) == all_single, "shape %d %d %d trip %d: rows %d", N, C, K, t, rows);
        CHECK(rows == 1 || rows == 2, "rows %d", rows);
        CHECK(srb_trip_all_rows_on(N, C, K, NTH, t) == all_on, "shape %d %d %d trip %d", N, C, K, t);
        CHECK(srb_trip_has_com(N, C, K, NTH, t) == any_com, "shape %d %d %d trip %d", N, C, K, t);
    }
}

static void run_time(int TS, int NW)
{
    const int NTH = 64 * NW;
    CHECK(srb_trips_cover(0, 0, 0, NTH, TS), "run-time shape");
    for (int t = 0; t < TS; t++) {
        CHECK(srb_trip_kinds(0, 0, 0, NTH, t) == SRB_KM_ANY, "trip %d", t);
        CHECK(srb_trip_rows(0, 0, 0, NTH, t) == 2, "trip %d", t);
        CHECK(!srb_trip_all_rows_on(0, 0, 0, NTH, t), "trip %d", t);
        CHECK(srb_trip_has_com(0, 0, 0, NTH, t), "trip %d", t);
    }
    // a shape with only some of its parameters compiled is a run-time shape too
    CHECK(srb_trip_kinds(10, 2, 0, NTH, 0) == SRB_KM_ANY && srb_trip_rows(10, 0, 11, NTH, 3) == 2, "partial shapes");
}

// the tables are usable where the kernel uses them: in constant expressions
static_assert(srb_trip_kinds(10, 2, 11, 64, 0) == SRB_KM(SRB_K_VAR), "12_4_1_10_2_11 trip 0 is VAR only");
static_assert(srb_trip_kinds(10, 2, 11, 64, 2) == SRB_KM(SRB_K_OBS), "12_4_1_10_2_11 trip 2 is OBS only");
static_assert(srb_trip_kinds(10, 2, 11, 64, 3) == (SRB_KM(SRB_K_OBS) | SRB_KM(SRB_K_NONE)), "12_4_1_10_2_11 trip 3");
static_assert(srb_trip_rows(10, 2, 11, 64, 1) == 2 && srb_trip_rows(10, 2, 11, 64, 2) == 1, "rows");
static_assert(srb_trips_cover(10, 2, 11, 64, 4) && !srb_trips_cover(10, 2, 11, 64, 3), "cover: 229 slots need 4 trips");

int main()
{
    compiled(4, 1, 10, 2, 11);      // 12_4_1_10_2_11
    compiled(1, 4, 10, 2, 3);       // 12_1_4_10_2_3
    compiled(4, 2, 20, 2, 11);      // 24_4_2_20_2_11
    run_time(4, 1);                 // 12_4_1_0_0_0
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("slot kinds ok\n");
    return 0;
}
