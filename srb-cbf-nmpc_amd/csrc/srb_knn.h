// K-nearest selection over a table of rows, brute force or through a uniform grid (srb_select.hip).  Header-only,
// device code.
#pragma once
#include "srb_kernel_decls.h"
#include "srb_wave.h"

// rows a lane holds in registers on the thresholded brute-force path of knn_select_k (larger tables: the
// batched scan); 32: the neighbour snapshot of a 2048-agent shard on one wave
#ifndef SRB_KNN_RB
#define SRB_KNN_RB 32
#endif

// per-lane insertion of candidate (cd = sqrt distance, ci = row) into the sorted top-K
// (bd, bi), ordered lexicographically by (distance, index)
template <int KM>
__device__ __forceinline__ void knn_insert(double (&bd)[KM], int (&bi)[KM], double cd, int ci, int K)
{
#pragma unroll
    for (int j = 0; j < KM; j++) {
        const bool lt = (j < K) && (cd < bd[j] || (cd == bd[j] && ci < bi[j]));
        const double td = bd[j]; const int ti = bi[j];
        bd[j] = lt ? cd : td; bi[j] = lt ? ci : ti;
        cd = lt ? td : cd; ci = lt ? ti : ci;
    }
}

template <int KW, int KM>
__device__ __forceinline__ void knn_pop(int tid, double (&bd)[KM], int (&bi)[KM], int K, int cap, int *sel,
                                        double *wd_lds, int *wi_lds);

// The thresholded brute-force pass of knn_select_k (round 6) over a table of at most RB rows a lane: every
// row's d^2 kept in registers (row tid + r STEP in slot r; NaN for the agent itself, rows past the table and
// rows with NaN coordinates, which are never selected), then a bound T on the K-th smallest d^2 from the lanes'
// minima -- the K-th smallest of them: at least K rows of this wave lie within it -- and only the rows with
// d^2 <= T (1 + 1e-14) (the filter's padding: a row beyond cannot round to a sqrt at or below the K-th's)
// enter the lanes' sorted lists, each lane taking its candidates one per trip.  The per-row insertion was
// three quarters of the neighbour scan (tools/ubench/knn_phase.hip); configs[2] selection 20.6 -> 14.5 us.
template <int KM, int RB, int STEP>
__device__ __forceinline__ void knn_thresh(int tid, double px, double py, const double *__restrict__ tab, int stride,
                                           int n_rows, int self, int K, double (&bd)[KM], int (&bi)[KM])
{
#pragma clang fp contract(off)
    double key[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) {
        const int i = tid + r * STEP;
        const bool in = i < n_rows;
        const double tx = in ? tab[(size_t)stride * i] : 0.0, ty = in ? tab[(size_t)stride * i + 1] : 0.0;
        const double dx = px - tx, dy = py - ty;
        key[r] = (in && i != self) ? dx * dx + dy * dy : __builtin_nan("");
    }
    double lm = __builtin_inf();
#pragma unroll
    for (int r = 0; r < RB; r++) lm = fmin(lm, key[r]);      // NaN keys ignored
    double T = __builtin_inf();
    for (int cnt = 0; cnt < K;) {                  // uniform: every lane holds the same t
        const double t = wmin(lm);
        if (!(t < __builtin_inf())) { T = __builtin_inf(); break; }
        cnt += __popcll(__ballot(lm == t));
        T = t;
        lm = (lm == t) ? __builtin_inf() : lm;
    }
    const double wT = (T < __builtin_inf()) ? T * (1.0 + 1e-14) : __builtin_inf();
    unsigned long long cm = 0;
#pragma unroll
    for (int r = 0; r < RB; r++)
        if (key[r] <= wT) cm |= 1ull << r;         // NaN keys fail
    while (__ballot(cm != 0)) {
        if (cm) {
            const int rr = __ffsll((long long)cm) - 1;
            cm &= cm - 1;
            double kd = key[0];
#pragma unroll
            for (int r = 1; r < RB; r++) kd = (rr == r) ? key[r] : kd;
            knn_insert<KM>(bd, bi, sqrt(kd), tid + rr * STEP, K);
        }
    }
}

// K nearest rows of a table (row i at tab[stride*i], x at +0, y at +1) to (px, py),
// ascending in (sqrt distance, index) -- the order of the reference's strict-'<' scan over
// sqrt(pow(dx,2)+pow(dy,2)) (MPC_dist.cpp:373-382; two rows whose squared distances differ
// but round to the same sqrt keep index order, as there) -- excluding row `self`; indices to
// sel[0..K).  cap != 0 applies the reference's min_dist = 1000 / min_i = 0 start: a round
// whose winner is not closer than 1000 m selects row 0.  NaN rows are never selected.
// KW waves (one workgroup) gather candidates -- every row (brute force), or with a grid the
// rows of the cells around the query that must hold the K nearest -- and each lane keeps a
// sorted top-K of its candidates; then K rounds pop the global order: a wave argmin over the
// lane heads, the KW wave winners through LDS (wd_lds, wi_lds: KW entries each), the owning
// lane drops its head (measured faster than per-wave pops followed by one merge of the KW K
// wave winners: two barriers per round cost less than K extra wave-argmin rounds).  The sqrt
// is taken only for rows that can enter a lane's list: d^2 above its K-th entry's squared key
// by more than a relative 1e-14 cannot round to a smaller sqrt.
template <int KW, int KM>
__device__ __forceinline__ void knn_select_k(int tid, double px, double py, const double *__restrict__ tab,
                                           int stride, int n_rows, int self, int K, int cap, int *sel,
                                           double *wd_lds, int *wi_lds, const SrbGrid *grid = nullptr,
                                           const int *__restrict__ cell_off = nullptr,
                                           const double2 *__restrict__ spos = nullptr,
                                           const int *__restrict__ sidx = nullptr)
{
#pragma clang fp contract(off)
    const int lane = tid & 63, wv = tid >> 6;
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { bd[j] = __builtin_inf(); bi[j] = 0x7fffffff; }
    double wq = __builtin_inf();                   // filter bound on d^2 (K-th key squared, padded)
    constexpr int STEP = 64 * KW;
    auto offer = [&](double tx, double ty, int i) {
        const double dx = px - tx, dy = py - ty;
        const double d2 = dx * dx + dy * dy;
        if (i == self || !(d2 <= wq)) return;
        knn_insert<KM>(bd, bi, sqrt(d2), i, K);
#pragma unroll
        for (int j = 0; j < KM; j++)
            if (j == K - 1) wq = bd[j] * bd[j] * (1.0 + 1e-14);
    };
    // ---- grid search: the smallest Chebyshev ring r0 of cells around the query cell holding
    // K candidates bounds the K-th distance by (r0 + 1) sqrt(2) h, so every row closer than
    // that lies in the ring R = ceil((r0 + 1) sqrt 2) + 1; queries far outside the grid (or a
    // grid that cannot supply K rows) fall back to the brute-force scan
    bool done = false;
    if (grid && grid->ok) {
        const SrbGrid g = *grid;
        const double fx = floor((px - g.x0) * g.inv_h), fy = floor((py - g.y0) * g.inv_h);
        const int keff = K + (self >= 0 ? 1 : 0);
        if (g.n >= keff && fx > -64.0 && fy > -64.0 && fx < g.nx + 64.0 && fy < g.ny + 64.0) {
            const int cx = (int)fx, cy = (int)fy, rmax = max(g.nx, g.ny) + 64;
            auto rows_in = [&](int r, int y) -> int {        // rows of cell-row y within x-range of ring r
                const int xl = max(cx - r, 0), xr = min(cx + r, g.nx - 1);
                if (y < 0 || y >= g.ny || xl > xr) return 0;
                return cell_off[y * g.nx + xr + 1] - cell_off[y * g.nx + xl];
            };
            // rings 0..3 in one pass (lane l < 16 counts cell row y = cy + l - r(r+1) of ring
            // r = floor(sqrt(l))), then ring by ring from 4 if none of them holds keff rows
            int r0 = 4;
            {
                const int rr = (lane < 1) ? 0 : (lane < 4) ? 1 : (lane < 9) ? 2 : (lane < 16) ? 3 : -1;
                const int v = (rr >= 0) ? rows_in(rr, cy + lane - rr * rr - rr) : 0;
#pragma unroll
                for (int r = 3; r >= 0; r--) {
                    int cr = (rr == r) ? v : 0;
                    for (int o = 32; o > 0; o >>= 1) cr += __shfl_xor(cr, o, 64);
                    if (cr >= keff) r0 = r;
                }
            }
            for (; r0 >= 4 && r0 < rmax; r0++) {            // uniform: every thread computes the same count
                int cnt = 0;
                for (int y = cy - r0 + lane; y <= cy + r0; y += 64) cnt += rows_in(r0, y);
                for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
                if (cnt >= keff) break;
            }
            if (r0 < rmax) {
                const int R = (int)ceil((r0 + 1) * 1.4142135623730951) + 1;
                const int ylo = max(cy - R, 0), yhi = min(cy + R, g.ny - 1);
                const int xl = max(cx - R, 0), xr = min(cx + R, g.nx - 1);
                // up to 64 cell rows at a time: lane y loads its row's range [a, a + len), a wave
                // scan numbers the candidates, and every thread takes candidates c, c + STEP, ..
                // (segment found by a binary search over the scan), so the cell-offset loads and
                // the row loads are two dependent round trips instead of two per cell row
                for (int yb = ylo; xl <= xr && yb <= yhi; yb += 64) {
                    const int y = yb + lane;
                    int a = 0, len = 0;
                    if (y <= yhi) { a = cell_off[y * g.nx + xl]; len = cell_off[y * g.nx + xr + 1] - a; }
                    int inc = len;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
                    const int total = __shfl(inc, 63, 64), exc = inc - len;
                    for (int c0 = 64 * wv; c0 < total; c0 += STEP) {      // wave-uniform trip count
                        const int c = c0 + lane;
                        int j = 0;                                        // last lane with exc <= c
#pragma unroll
                        for (int st = 32; st > 0; st >>= 1) j += (__shfl(exc, j + st, 64) <= c) ? st : 0;
                        const int i = __shfl(a, j, 64) + (c - __shfl(exc, j, 64));
                        if (c < total) {
                            const double2 q = spos[i];
                            offer(q.x, q.y, sidx[i]);
                        }
                    }
                }
                done = true;
            }
        }
    }
    if (!done && n_rows <= STEP * SRB_KNN_RB) {
        // ---- brute force with a threshold (knn_thresh), as many register slots as the table needs
        if (n_rows <= STEP * 4) knn_thresh<KM, 4, STEP>(tid, px, py, tab, stride, n_rows, self, K, bd, bi);
        else if (n_rows <= STEP * 16) knn_thresh<KM, 16, STEP>(tid, px, py, tab, stride, n_rows, self, K, bd, bi);
        else knn_thresh<KM, SRB_KNN_RB, STEP>(tid, px, py, tab, stride, n_rows, self, K, bd, bi);
        done = true;
    }
    if (!done) {
        // ---- brute force: KNN_U rows per lane per batch, all loads issued before the first use
#ifndef SRB_KNN_U
#define SRB_KNN_U 4
#endif
        constexpr int KNN_U = SRB_KNN_U;
        for (int i0 = tid; i0 < n_rows; i0 += KNN_U * STEP) {
            double tx[KNN_U], ty[KNN_U];
#pragma unroll
            for (int u = 0; u < KNN_U; u++) {
                const int i = i0 + u * STEP;
                const bool in = i < n_rows;
                tx[u] = in ? tab[(size_t)stride * i] : 0.0;
                ty[u] = in ? tab[(size_t)stride * i + 1] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < KNN_U; u++)
                if (i0 + u * STEP < n_rows) offer(tx[u], ty[u], i0 + u * STEP);
        }
    }
    knn_pop<KW, KM>(tid, bd, bi, K, cap, sel, wd_lds, wi_lds);
}

// The K pop rounds over the lanes' sorted lists (knn_select_k, and srb_knn_plan_kernel's lists keyed by closest
// predicted approach): the global (distance, index) order into sel[0..K).
template <int KW, int KM>
__device__ __forceinline__ void knn_pop(int tid, double (&bd)[KM], int (&bi)[KM], int K, int cap, int *sel,
                                        double *wd_lds, int *wi_lds)
{
    const int lane = tid & 63, wv = tid >> 6;
    // round j's winner is kept by lane j and stored after the last round: a store inside the
    // loop would make every barrier wait for it (s_waitcnt vmcnt(0) before s_barrier)
    int mine = -1;
#pragma clang loop unroll(disable)
    for (int j = 0; j < K; j++) {
        double d = bd[0]; int idx = bi[0];
        wargmin_b(d, idx);
        if (KW > 1) {
            if (lane == 0) { wd_lds[wv] = d; wi_lds[wv] = idx; }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < KW; w++) {
                const double od = wd_lds[w]; const int oi = wi_lds[w];
                if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
            }
            __syncthreads();                       // every wave has read the winners
        }
        if (bi[0] == idx) {
#pragma unroll
            for (int t = 0; t + 1 < KM; t++) { bd[t] = bd[t + 1]; bi[t] = bi[t + 1]; }
            bd[KM - 1] = __builtin_inf(); bi[KM - 1] = 0x7fffffff;
        }
        if (tid == j) mine = cap ? ((d < 1000.0) ? idx : 0) : ((idx == 0x7fffffff) ? -1 : idx);
    }
    if (tid < K) sel[tid] = mine;
}
// the insertion network as deep as K needs (K <= KM): 4, 8 or SRB_KNN_MAX entries
template <int KW>
__device__ __forceinline__ void knn_select(int tid, double px, double py, const double *__restrict__ tab,
                                           int stride, int n_rows, int self, int K, int cap, int *sel,
                                           double *wd_lds, int *wi_lds, const SrbGrid *grid = nullptr,
                                           const int *cell_off = nullptr, const double2 *spos = nullptr,
                                           const int *sidx = nullptr)
{
    if (K <= 4) knn_select_k<KW, 4>(tid, px, py, tab, stride, n_rows, self, K, cap, sel, wd_lds, wi_lds, grid, cell_off, spos, sidx);
    else if (K <= 8) knn_select_k<KW, 8>(tid, px, py, tab, stride, n_rows, self, K, cap, sel, wd_lds, wi_lds, grid, cell_off, spos, sidx);
    else knn_select_k<KW, SRB_KNN_MAX>(tid, px, py, tab, stride, n_rows, self, K, cap, sel, wd_lds, wi_lds, grid, cell_off, spos, sidx);
}

// The scan of the horizon-aware selection (srb_knn_plan_kernel; srb_knn_plan_scene_kernel on a scene's rows): the
// K rows of n_all of closest predicted approach to the agent whose N + 1 points are own[] (its snapshot position,
// then its plan), row `self` left out.  Every thread of the SRB_KNN_PLAN_WAVES waves scans rows tid,
// tid + 64 KW, .. and keeps a sorted list (knn_insert); knn_pop merges them into sel[0..K).
template <int KM>
__device__ __forceinline__ void knn_plan_select(int tid, const double *own, const double *__restrict__ nbr_state,
                                                const double *__restrict__ nbr_plan, int n_all, int N, int self, int K,
                                                int *sel, double *wd_lds, int *wi_lds)
{
#pragma clang fp contract(off)
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { bd[j] = __builtin_inf(); bi[j] = 0x7fffffff; }
    double wq = __builtin_inf();                   // filter bound on the squared key (knn_select_k's)
    for (int i = tid; i < n_all; i += 64 * SRB_KNN_PLAN_WAVES) {
        if (i == self) continue;
        const double *row = nbr_plan + 2 * (size_t)i * N;
        const double dx0 = own[0] - nbr_state[4 * (size_t)i], dy0 = own[1] - nbr_state[4 * (size_t)i + 1];
        double m = dx0 * dx0 + dy0 * dy0;
        for (int k = 0; k < N; k++) {
            const double dx = own[2 * k + 2] - row[2 * k], dy = own[2 * k + 3] - row[2 * k + 1];
            const double d2 = dx * dx + dy * dy;
            m = (d2 < m || d2 != d2) ? d2 : m;       // the minimum; a NaN pair makes the key NaN for good
        }
        if (!(m <= wq)) continue;                  // NaN keys fail: such rows are never selected
        knn_insert<KM>(bd, bi, sqrt(m), i, K);
#pragma unroll
        for (int j = 0; j < KM; j++)
            if (j == K - 1) wq = bd[j] * bd[j] * (1.0 + 1e-14);
    }
    knn_pop<SRB_KNN_PLAN_WAVES, KM>(tid, bd, bi, K, 0, sel, wd_lds, wi_lds);
}

// The scan of the horizon-aware obstacle selection (srb_knn_obs_horizon_kernel; its scene form on a scene's rows):
// the K rows of n_obs of closest predicted approach to the agent whose N + 1 constant-velocity points are own[]
// (point k at time Ts k).  The key of row i is sqrt(min_k d_k^2), the obstacle of pair k at o + w (Ts k), w its
// obs_vel row -- for k >= 1 the bits of the rows the solve builds (SRB_AGENT_OBSTACLES).  Every thread of the
// SRB_KNN_OBS_WAVES waves scans rows tid, tid + 64 KW, .. and keeps a sorted list (knn_insert); knn_pop merges them
// into sel[0..K) with the static table's 1000 m rule (cap = 1).
template <int KM>
__device__ __forceinline__ void knn_obs_horizon_select(int tid, const double *own, const double *__restrict__ obstacles,
                                                       const double *__restrict__ obs_vel, int n_obs, int N, double Ts,
                                                       int K, int *sel, double *wd_lds, int *wi_lds)
{
#pragma clang fp contract(off)
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; j++) { bd[j] = __builtin_inf(); bi[j] = 0x7fffffff; }
    double wq = __builtin_inf();                   // filter bound on the squared key (knn_select_k's)
    for (int i = tid; i < n_obs; i += 64 * SRB_KNN_OBS_WAVES) {
        const double ox = obstacles[2 * (size_t)i], oy = obstacles[2 * (size_t)i + 1];
        const double wx = obs_vel[2 * (size_t)i], wy = obs_vel[2 * (size_t)i + 1];
        double m = __builtin_inf();
        for (int k = 0; k <= N; k++) {
            const double tk = Ts * (double)k;
            const double dx = own[2 * k] - (ox + wx * tk), dy = own[2 * k + 1] - (oy + wy * tk);
            const double d2 = dx * dx + dy * dy;
            m = (d2 < m || d2 != d2) ? d2 : m;       // the minimum; a NaN pair makes the key NaN for good
        }
        if (!(m <= wq)) continue;                  // NaN keys fail: such rows are never selected
        knn_insert<KM>(bd, bi, sqrt(m), i, K);
#pragma unroll
        for (int j = 0; j < KM; j++)
            if (j == K - 1) wq = bd[j] * bd[j] * (1.0 + 1e-14);
    }
    knn_pop<SRB_KNN_OBS_WAVES, KM>(tid, bd, bi, K, 1, sel, wd_lds, wi_lds);
}
