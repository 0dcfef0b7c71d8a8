// The body of one solve stage of nmpc_agent (srb_kernels.hip): set-up, interior-point iterations, the stage's flag.
// No header in the usual sense: a piece of nmpc_agent's text, included inside that function once per compiled copy of
// the stage -- three times, so that the compiler sees the same text each time and no call, closure or reference
// stands between the body and the function's state:
//   - in the one loop over the two stages (`stage` the loop variable, `nl = stage == 1` at run time), the form of
//     every run-time shape and of NZL > 16;
//   - twice in the split form of the compiled one-column-block shapes (SPLIT), with `stage` / `nl` constexpr 0 / false
//     and 1 / true, each inside a `do { .. } while (0)`.
// The including scope provides `stage` and `nl`.  The one `continue` (the QP set-up's factor failure) leaves the stage
// in either form: in the loop it goes to the next stage, in a do-while (0) to the false condition.
        // the QP stage that the NLP follows runs to qp_warm_tol (its point is only the NLP's warm start)
        const double tolS = (!nl && prm.use_nlp && prm.qp_warm_tol > 0.0) ? prm.qp_warm_tol : tol, thS = tolS / sqrt(3.0);
        STAMP_STAGE(stage);
        const int nts = ((nl ? S : sV) + NTH - 1) / NTH;      // active slot trips
        const int mrows = nl ? (4 * (N - 1) + 12 * N + 2 * C * N + NK + 4 * N) : (4 * (N - 1) + 12 * N + 2 * C * N);
        const int cnt = rU, nko = nl ? NKP : 0;            // MFMA term rows (X, CoM-CoP), obstacle terms
        STAMP_BEGIN();
        // stage activity of each row
        // (written out here rather than through slot_stage: the call form measurably changes the
        // register allocation of the whole loop, 8 -> 72 VGPR spills for 12_4_1)
#pragma unroll
        for (int t = 0; t < TS; t++) {
            Slot &q = Q[t];
            const bool lin = (SK_ISP(q, t, K_VAR) && (SK_ON(t) || q.i0 < n - 1)) || SK_ISP(q, t, K_COP);
            q.m[0] = (lin || (nl && (SK_ISP(q, t, K_VEL) || SK_ISP(q, t, K_OBS)))) ? 1.0 : 0.0;
            q.m[1] = (lin || (nl && SK_ISP(q, t, K_VEL))) ? 1.0 : 0.0;
            q.wr = (SK_ISP(q, t, K_VAR) || SK_ISP(q, t, K_COP) || SK_ISP(q, t, K_OBS)) ? q.r : TT;
        }
        if (!nl) {
            // ---------------- QP stage setup: kkt_initialize (Auxilary.c:680-755) ----------------
            // [P A' G'; A 0 0; G 0 -I] [x; y; z] = [-c; b; h]:  (Z'(P + G'G)Z) xi = -Z'(P xbar + c) + Z'G'(h - G xbar)
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (SK_TWO(t) && t < nts) {                 // (a single-row trip holds no QP row)
                    Slot &q = Q[t];
                    const double f = slot_f<TK>(q, t, xs, 0.0);
                    const double w0 = SK_M(q, t, 0) * (q.h[0] - f), w1 = SK_M(q, t, 1) * (q.h[1] + f);
                    const bool var = SK_ISP(q, t, K_VAR);
                    const double wgt = (var ? q.a0 : 0.0) + SK_M(q, t, 0) + SK_M(q, t, 1);
                    const double cfv = (var ? -q.a1 - q.a0 * f : 0.0) + (w0 - w1);
                    if (SK_ISP(q, t, K_VAR) || SK_ISP(q, t, K_COP)) { W[q.r] = wgt; CF[q.r] = cfv; }
                }
            SYNC();
            if constexpr (GVEC) gram_rhs_vec<NZL, true, GSH, SRB_GRAM_FORM>(R, W, CF, OF, nko, H0, vg, nz, lane);
            else gram_rhs<NZL, true, NW>(R, W, CF, cnt, OF, nko, H0, vg, nz, tid, part, bmask);
            SYNC();
            gj_load<NZL, NZE>(Mi, H0, ZZ, 0.0, nz, lane);
            if (gj_factor<NZL, NZE>(Mi, nz, lane, 1) != 0) {
                qp_flag = 1;                                  // x stays xbar (last iterate is returned)
                continue;
            }
            la_solve<NZL, NW, NZE>(Mi, H0, ZZ, 0.0, vg, vy, vr, vd, dxi, nz, lane);
            // x = xbar + Z xi ; zi = h - G x ; s, z shifted (Auxilary.c:716-746)
            double mn = 1e300, mx = -1e300;
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (SK_TWO(t) && t < nts) {
                    Slot &q = Q[t];
                    const double f = slot_f<TK>(q, t, xs, 0.0) +
                        ((!SRB_OBS_STORED(NZL) && SK_ISP(q, t, K_OBS)) ? 0.0 : row_dot<NZL, NZE>(R + q.r * LDR, dxi));   /* (OBS: masked here) */
                    q.jd = f;                                 // f(x) for the shift below
                    const double z0 = q.h[0] - f, z1 = q.h[1] + f;
                    if (SK_M(q, t, 0) != 0.0) { mn = fmin(mn, z0); mx = fmax(mx, z0); }
                    if (SK_M(q, t, 1) != 0.0) { mn = fmin(mn, z1); mx = fmax(mx, z1); }
                }
            double rv[2] = {-mn, mx};
            wred_x<2, 3u, NW>(rv, red + 0 * 8 * NW, tid);
            mn = -rv[0]; mx = rv[1];
            const double ssh = (-mn < 0) ? 0.0 : 1.0 - mn, zsh = (mx < 0) ? 0.0 : 1.0 + mx;
            SYNC();                                           // every lane has read xs = xbar
            // qp_init 1 (default): the scaled start of oracle/qp_ipm.c, s = max(h - Gx, 0.1), z = 1/s
            // (iSWIFT's z shift by 1 + max(h - Gx) is ~1e3 with the +-1e3 boxes: blocked dual steps,
            // up to 19 iterations on the bench batch against 9); qp_init 0: iSWIFT's start
            const bool scaled = prm.qp_init == 1;
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (SK_TWO(t) && t < nts) {
                    Slot &q = Q[t];
                    const double f = q.jd, z0 = q.h[0] - f, z1 = q.h[1] + f;
                    q.s[0] = (SK_M(q, t, 0) != 0.0) ? (scaled ? fmax(z0, 0.1) : z0 + ssh) : 1.0;
                    q.s[1] = (SK_M(q, t, 1) != 0.0) ? (scaled ? fmax(z1, 0.1) : z1 + ssh) : 1.0;
                    q.z[0] = (SK_M(q, t, 0) != 0.0) ? (scaled ? rcp_d(q.s[0]) : -z0 + zsh) : 1.0;
                    q.z[1] = (SK_M(q, t, 1) != 0.0) ? (scaled ? rcp_d(q.s[1]) : -z1 + zsh) : 1.0;
                    if (SK_ISP(q, t, K_VAR)) xs[q.i0] = f;
                    // rx = -(P x + c + A'y + G'z) = -G'(z - (G x - h)) at the least-squares start: 0 for
                    // iSWIFT's z (the shift is the same on the two rows of every +- pair), below for the
                    // scaled one (each row's z + (h - Gx) scattered onto its variables)
                    q.rx = 0.0;
                }
            if (scaled) {
                SYNC();
#pragma unroll
                for (int t = 0; t < TS; t++)              // the VAR rows' own bounds first (plain stores)
                    if (t < nts && SK_ISP(Q[t], t, K_VAR)) {
                        const Slot &q = Q[t];
                        CF[q.r] = SK_M(q, t, 0) * (q.z[0] + q.h[0] - q.jd) - SK_M(q, t, 1) * (q.z[1] + q.h[1] + q.jd);
                    }
                SYNC();
#pragma unroll
                for (int t = 0; t < TS; t++)              // CoM-CoP rows +-(p_i - u_i+1): onto p_i and u_i+1
                    if (t < nts && SK_ISP(Q[t], t, K_COP)) {
                        const Slot &q = Q[t];
                        const double g = q.m[0] * (q.z[0] + q.h[0] - q.jd) - q.m[1] * (q.z[1] + q.h[1] + q.jd);
                        __hip_atomic_fetch_add(&CF[TL.zr(q.i0)], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(&CF[TL.zr(q.i1)], -g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                SYNC();
#pragma unroll
                for (int t = 0; t < TS; t++)
                    if (t < nts && SK_ISP(Q[t], t, K_VAR)) Q[t].rx = -CF[Q[t].r];
            }
            SYNC();
            STAMP_END(1);
        } else {
            // ---------------- NLP stage setup (replaces SnoptSolver::Solve, MPC_dist.cpp:402-427) ----------------
            if (x_qp_out)
                for (int v = tid; v < n; v += NTH) x_qp_out[(size_t)agent * n + v] = xs[v];
            // obstacles per grid: the K_obs nearest static obstacles (MPC_dist.cpp:371-396,
            // generalised to K) and the K_nbr nearest other agents (get_lastState() rows),
            // predicted at constant velocity o_k = p + v Ts (k+1); query point = own CoM.
            // (selected by srb_knn_kernel, launched just before this kernel on the same stream)
            STAMP_END(6);                                     // NLP slot 6 (obstacle positions: loaded in the setup)
            SYNC();
            // slacks: shifted h - g(x) over every NLP row; duals 1
            const double s_var = xs[n - 1];
            double mn = 1e300;
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (t < nts) {
                    Slot &q = Q[t];
                    if (SK_ISP(q, t, K_OBS)) {
                        const int o = tid + NTH * t - sO;
                        LCK(o >= 0 && o < NK, 5);
                        q.a0 = obs[2 * o]; q.a1 = obs[2 * o + 1]; q.h[0] = -eps[o % K];
                    }
                    const double f = slot_f<TK>(q, t, xs, s_var);
                    q.jd = f;
                    if (SK_M(q, t, 0) != 0.0) mn = fmin(mn, q.h[0] - f);
                    if (SK_M(q, t, 1) != 0.0) mn = fmin(mn, q.h[1] + f);
                }
            {
                double rv[1] = {-mn};
                wred_x<1, 1u, NW>(rv, red + 1 * 8 * NW, tid);
                mn = -rv[0];
            }
            const double ssh = (-mn < 0) ? 0.0 : 1.0 - mn;
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (t < nts) {
                    Slot &q = Q[t];
                    const double f = q.jd;
                    q.s[0] = (SK_M(q, t, 0) != 0.0) ? q.h[0] - f + ssh : 1.0;
                    if (SK_TWO(t)) q.s[1] = (SK_M(q, t, 1) != 0.0) ? q.h[1] + f + ssh : 1.0;
                    // z = Z0 / max(s, 1): rows far from their bound start at complementarity Z0, the
                    // others at Z0 (oracle/nlp_ipm.c, same rule)
                    q.z[0] = SRB_NLP_Z0 * rcp_d(fmax(q.s[0], 1.0));
                    if (SK_TWO(t)) q.z[1] = SRB_NLP_Z0 * rcp_d(fmax(q.s[1], 1.0));
                    if (SK_ISP(q, t, K_OBS)) {                     // M_o = J_o Z at the current x (gram_rhs)
                        const int o = q.r - rO;
                        obs_relin<NZL>(R, OJ, rO, o, q.i0, q.i1, -2.0 * (xs[q.i0] - q.a0), -2.0 * (xs[q.i1] - q.a1));
                    }
                    // Z'Z (delta shifts) and rx0 = -Z (Z'Z)^-1 Z'(P x + c + J'z): each row's J'z on its
                    // term row (the velocity rows' below, onto their variables' rows)
                    const double jz = SK_TWO(t) ? SK_M(q, t, 0) * q.z[0] - SK_M(q, t, 1) * q.z[1] : q.m[0] * q.z[0];
                    if (SK_ISP(q, t, K_VAR)) { W[q.r] = 1.0; CF[q.r] = fma(q.a0, f, q.a1) + jz; }
                    else if (SK_ISP(q, t, K_COP)) { W[q.r] = 0.0; CF[q.r] = jz; }
                    else if (SK_ISP(q, t, K_OBS)) { W[q.r] = 0.0; CF[q.r] = q.z[0]; }
                }
            if (NW > 1) SYNC();                               // the VAR rows' plain stores land before the VEL adds
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (t < nts && SK_ISP(Q[t], t, K_VEL))
                    __hip_atomic_fetch_add(&CF[Q[t].r], Q[t].m[0] * Q[t].z[0] - Q[t].m[1] * Q[t].z[1], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
            SYNC();
            // the first write of ZZ: the obstacle positions it may alias (SRB_OBS_IN_ZZ) were read by the slots'
            // setup above, and until here every ZZ operand was scaled by a zero shift, never read (gj_load / la_solve
            // test delta != 0; the LDS-check build asserts it, bit 7)
            if constexpr (GVEC) gram_rhs_vec<NZL, true, GSH, SRB_GRAM_FORM>(R, W, CF, OF, nko, ZZ, vg, nz, lane);
            else gram_rhs<NZL, true, NW>(R, W, CF, cnt, OF, nko, ZZ, vg, nz, tid, part, bmask);
            SYNC();
            gj_load<NZL, NZE>(Mi, ZZ, ZZ, 0.0, nz, lane);
            gj_factor<NZL, NZE>(Mi, nz, lane, 0);
            la_solve<NZL, NW, NZE>(Mi, ZZ, ZZ, 0.0, vg, vy, vr, vd, dxi, nz, lane);
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (t < nts) {
                    Slot &q = Q[t];
                    q.rx = (SK_ISP(q, t, K_VAR)) ? -row_dot<NZL, NZE>(R + q.r * LDR, dxi) : 0.0;
                }
            SYNC();
            STAMP_END(2);
        }

        // =============================== interior-point iterations ===============================
        const int maxit = nl ? prm.nlp_maxit : prm.qp_maxit;
        double sigma = 100.0;            // options->sigma = SIGMA
        const double sigma_d = 0.0;
        int flag = 2, it = 0;
        const double inv_m = 1.0 / (double)mrows;
        double dxl = 1e300;              // this lane's max |ap dx| over its variable slots, last update
        int npassed = 0;                 // NLP: near-optimal iterates so far
        bool saved = false, restore = false;   // NLP: xsv holds the best near-optimal iterate
        bool prov = false;                     // NLP: OPTIMAL by the loosened tests only (-> 4 until polished)
        double best_rx = 1e300;                // its dual residual / max(1, ||Q x + f||_inf)
        // the polish kernel (srb_polish_kernel, launched next) starts from the NLP result: its active
        // set and multipliers -- rows with s * KAPPA < z keep z (as float: the Newton iteration's
        // starting guess, corrected by its first step; measured no different from double), the
        // others -min(z/s, OMCAP), their barrier weight, as a proximal term
        // -- go to HBM, zpol_g[agent][2 slot + row], with the iterate the result is taken from
        // (the saved one on a restore)
        // (LDS or global by a uniform branch, not a pointer select: a generic pointer would make these flat stores)
        auto export_zpol = [&]() {
            const bool to_lds = SRB_FUSED_POLISH_OK(NZL) && prm.polish_fused;
            // address-space-typed pointers: the two stores cannot be merged into one through a select
            __attribute__((address_space(1))) float *zg = (__attribute__((address_space(1))) float *)(zpol_g + (size_t)agent * zstride);
            __attribute__((address_space(3))) float *zl = (__attribute__((address_space(3))) float *)zpl;
#pragma unroll
            for (int t = 0; t < TS; t++)
                if (t < nts && tid + NTH * t < S)
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        const float v = SK_M(Q[t], t, r) == 0.0 ? 0.0f
                            : (float)(Q[t].s[r] * SRB_POLISH_KAPPA < Q[t].z[r] ? Q[t].z[r] : -fmin(Q[t].z[r] / Q[t].s[r], SRB_POLISH_OMCAP));
                        if (to_lds) zl[2 * (tid + NTH * t) + r] = v;
                        else zg[2 * (tid + NTH * t) + r] = v;
                    }
        };
        for (int v = tid; v < n; v += NTH) xprev[v] = xs[v];
        // compiled shapes, NLP: sum_j z_kj of the grid whose CoM position this lane's VAR slot holds, formed once an
        // iteration -- by the update, from the new duals -- and carried to the next iteration's weights and update
        // (iteration 0: by the weights phase); only the trips that hold such slots (TK::com) keep a register
        double hsc[TS] = {};
        for (int iter = 0; iter < maxit; iter++) {
            STAMP_BEGIN();
            // ---- residuals (computeresiduals, Auxilary.c:524-553), norms, reciprocals
            const double s_var = xs[n - 1];
            double nrx = 0.0, nrz = 0.0, sz = 0.0, gm = 1.0, zmx = 0.0;
            double fv[TS];
            double xa[TS], xc[TS];                            // xs[i0], xs[i1] of every slot, loaded together
#pragma unroll
            for (int t = 0; t < TS; t++) {
                xa[t] = xc[t] = 0.0;
                if (t < nts) { xa[t] = xs[Q[t].i0]; xc[t] = xs[Q[t].i1]; }
            }
#pragma unroll
            for (int t = 0; t < TS; t++) {
                fv[t] = 0.0;
                if (t < nts) {
                    Slot &q = Q[t];
                    const double f = slot_fx<TK>(q, t, xa[t], xc[t], s_var);
                    fv[t] = f;
                    if (SK_IS(q, t, K_VAR)) {
                        nrx = fma(q.rx, q.rx, nrx);
                        gm = fmax(gm, fabs(fma(q.a0, f, q.a1)));
                    }
                    const double m0 = SK_M(q, t, 0), m1 = SK_M(q, t, 1);
                    const double rz0 = q.h[0] - q.s[0] - f;
                    if (SK_TWO(t)) {
                        const double rz1 = q.h[1] - q.s[1] + f;
                        nrz = fma(m0 * rz0, rz0, fma(m1 * rz1, rz1, nrz));
                        sz = fma(m0 * q.s[0], q.z[0], fma(m1 * q.s[1], q.z[1], sz));
                        zmx = fmax(zmx, fmax(m0 * q.z[0], m1 * q.z[1]));
                    } else {                                  // single-row trip: the row-1 terms are 0 (m[1] = 0)
                        nrz = fma(m0 * rz0, rz0, nrz);
                        sz = fma(m0 * q.s[0], q.z[0], sz);
                        zmx = fmax(zmx, m0 * q.z[0]);
                    }
                    if constexpr (!LEAN)
#pragma unroll
                        for (int r = 0; r < 2; r++)
                            if (SK_TWO(t) || r == 0) { q.iz[r] = rcp_d(q.z[r]); q.is[r] = rcp_d(q.s[r]); }
                    if (nl && SK_IS(q, t, K_OBS)) {              // re-linearise: M_o = J_o(x) Z (gram_rhs)
                        const int o = q.r - rO;
                        obs_relin<NZL>(R, OJ, rO, o, q.i0, q.i1, -2.0 * (xa[t] - q.a0), -2.0 * (xc[t] - q.a1));
                        zo[o] = q.z[0];
                    }
                }
            }
            STAMP_END(18);                                    // stamps build: residual loop | reduction
            double dxm;
            {
                double rv[6] = {nrx, nrz, sz, gm, dxl, zmx};
                wred_x<6, 56u, NW>(rv, red + 2 * 8 * NW, tid);
                nrx = sqrt(rv[0]); nrz = sqrt(rv[1]); sz = rv[2]; gm = rv[3]; dxm = rv[4]; zmx = rv[5];
            }
            const double mu = sz * inv_m;
            const bool f32 = KF && mu > prm.kkt32_mu;          // KF instances: fp32 factor this iteration
            (void)f32;
            STAMP_END(3);
            // divergence: a dual beyond SRB_Z_DIV means infeasible rows (converging solves keep their duals
            // below ~1e4; infeasible ones pass 1e10 within a few iterations and then overflow): FATAL at
            // this finite iterate (oracle/qp_ipm.c, nlp_ipm.c: the same rule).  A non-finite iterate
            // (nothing else should produce one) returns the previous iterate, so no FATAL solve hands the
            // caller NaN or inf
            if (!isfinite(nrx) || !isfinite(nrz) || !isfinite(sz) || !(zmx <= SRB_Z_DIV)) {
                flag = 3;
                if (!isfinite(nrx) || !isfinite(nrz) || !isfinite(sz)) {
                    SYNC();
                    for (int v = tid; v < n; v += NTH) xs[v] = xprev[v];
                    SYNC();
                }
                break;
            }
            // NLP: dual residual scaled by max(1, ||Q x + f||_inf) (QP: iSWIFT's absolute test)
            const double thx = nl ? SRB_NLP_EXITF * th * gm : thS;
            const double mtol = nl ? SRB_NLP_EXITF * tol : tolS;
            NLPDBG(iter, 0, nrx); NLPDBG(iter, 1, thx); NLPDBG(iter, 2, nrz); NLPDBG(iter, 3, sz * inv_m);
            const bool pass = nrx < thx && nrz < thS && sz * inv_m < mtol;
            if (pass && (!nl || dxm < SRB_NLP_DXTOL)) {
                // NLP: met only by the loosened tests (SRB_NLP_EXITF, which rely on the polish), the result
                // is provisional -- ACCEPTABLE (4) unless the polish kernel accepts its polish (oracle, same rule)
                prov = nl && !(nrx < th * gm && sz * inv_m < tol);
                flag = 0; break;
            }
            // NLP near the optimum (primal and complementarity met, dual residual within 100x):
            // an inertia shift or a blocked step from here is round-off of the condensed
            // system (W = z/s ~ 1e14 swamps the soft curvature in Z'HZ), not progress -> exit
            // ACCEPTABLE (4) at this iterate (oracle/nlp_ipm.c, the same rule)
            const bool near = nl && nrz < th && sz * inv_m < mtol && nrx < 100.0 * thx;
            // a solve that reached the near-optimal region and then left it is past its round-off
            // floor: ACCEPTABLE at the best near-optimal iterate (oracle, same rule)
            if (nl && saved && !near) { restore = true; flag = 4; break; }
            if (near && nrx / gm <= best_rx) {     // each thread copies the variables it owns
                best_rx = nrx / gm;
                for (int v = tid; v < n; v += NTH) xsv[v] = xs[v];
                if (zpol_g || prm.polish_fused) export_zpol();
                saved = true;
            }
            if (near && ++npassed >= SRB_NLP_NEARWAIT) { flag = 4; break; }
            bool acc = false;
            const bool pc = nl || (sigma > sigma_d);
            double delta = 0.0;
            // right-hand side of pass (0 predictor, 1 corrector / centring):
            //   dsT, r3 = rz - dsT / z, w = om r3, coefficient of term row r = rx + J'w
            // RSL (srb_rhs_slots; with SPLIT the stage is a compile-time fact): pass 1 keeps each slot's coefficient in a
            // register for rhs_slots -- no CF store, no VEL atomic; pass 0 keeps its stores: the Gram reads them.  The
            // register is the slot's q.jd, which holds nothing between here and the J dx pass that rewrites it (so the
            // instances that keep rhs_only declare nothing new, and compile to the code they had)
            constexpr bool RSLS = RSL && (nl || SRB_RHS_SLOTS_QP);
            auto set_rhs = [&](int pass) {
                const double smu = (pass == 0) ? 0.0 : (pc ? sigma * mu : sigma_d * mu);
                const bool corr = pass == 1 && pc;
                double cfs[TS];
#pragma unroll
                for (int t = 0; t < TS; t++) {
                    cfs[t] = 0.0;
                    if (t < nts) {
                        Slot &q = Q[t];
                        const double f = fv[t];
                        double cf = (SK_IS(q, t, K_VAR)) ? q.rx : 0.0;
#pragma unroll
                        for (int r = 0; r < 2; r++)
                            if (SK_TWO(t) || r == 0) {
                                double dsT = -q.s[r] * q.z[r];
                                if constexpr (SPLIT) {
                                    // the three roundings written out -- the product, the fused corrector term, the
                                    // plain sum: in the NLP's own copy corr and smu are no longer behind a select, and
                                    // left to the compiler -s z - ds dz + sigma mu contracts differently there
                                    if (corr) dsT = fma(-q.ds[r], q.dz[r], dsT);
                                    dsT = add_plain(dsT, smu);
                                } else {
                                    if (corr) dsT -= q.ds[r] * q.dz[r];
                                    dsT += smu;
                                }
                                const double rz = r ? (q.h[1] - q.s[1] + f) : (q.h[0] - q.s[0] - f);
                                const double r3 = fma(-dsT, IZ(q, r), rz);
                                if constexpr (!LEAN) { q.dsT[r] = dsT; q.r3[r] = r3; }
                                cf = fma((r ? -SK_M(q, t, 1) : SK_M(q, t, 0)) * q.z[r] * IS(q, r), r3, cf);
                            }
                        cfs[t] = cf;
                        if constexpr (RSLS) { if (pass != 0) { q.jd = cf; continue; } }
                        CF[q.wr] = cf;
                    }
                }
                if constexpr (RSLS) { if (pass != 0) return; }
                if (NW > 1) SYNC();             // other waves' plain stores land before the VEL adds
                if (nl)
#pragma unroll
                    for (int t = 0; t < TS; t++)
                        if (t < nts && SK_IS(Q[t], t, K_VEL))
                            __hip_atomic_fetch_add(&CF[Q[t].r], cfs[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            if (pc) {
                // ---- weights W^-1 = z/s (updatekktmatrix, Auxilary.c:197-205), Lagrangian
                //      Hessian -2 sum_j z_kj on (x_k, y_k) (NLP), and the predictor right-hand
                //      side; one pass over the term rows assembles Z'HZ and Z'(rx + J'w)
                SYNC();
#pragma unroll
                for (int t = 0; t < TS; t++)
                    if (t < nts) {
                        Slot &q = Q[t];
                        const double om = SK_TWO(t) ? fma(SK_M(q, t, 0) * q.z[0], IS(q, 0), SK_M(q, t, 1) * q.z[1] * IS(q, 1))
                                                     : q.m[0] * q.z[0] * IS(q, 0);
                        double hs = 0.0;
                        if (nl && SK_COM(t) && SK_IS(q, t, K_VAR) && q.i0 < 4 * N && !(q.i0 & 1)) {
                            const int k = q.i0 >> 2;
                            // compiled shapes: the sum is carried from the previous iteration's update (hsc)
                            if constexpr (TK::compiled) {
                                if (iter == 0) hsc[t] = zo_sum(zo, k, K);
                                hs = hsc[t];
                            } else {
                                hs = zo_sum(zo, k, K);
                            }
                            hs *= -2.0;
                        }
                        W[q.wr] = om + ((SK_IS(q, t, K_VAR)) ? q.a0 + hs : 0.0);
                    }
                if (NW > 1) SYNC();
                if (nl)
#pragma unroll
                    for (int t = 0; t < TS; t++)
                        if (t < nts && SK_IS(Q[t], t, K_VEL))
                            __hip_atomic_fetch_add(&W[Q[t].r], Q[t].z[0] * IS(Q[t], 0) + Q[t].z[1] * IS(Q[t], 1), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                STAMP_END(16);
                set_rhs(0);
                SYNC();
                STAMP_END(17);
                if constexpr (GVEC) gram_rhs_vec<NZL, true, GSH, SRB_GRAM_FORM>(R, W, CF, OF, nko, H0, vg, nz, lane);
                else gram_rhs<NZL, true, NW>(R, W, CF, cnt, OF, nko, H0, vg, nz, tid, part, bmask);
                SYNC();
                STAMP_END(4);
                int ok = 0;
                const int ntries = nl ? 14 : 1;
                for (int tries = 0; tries < ntries; tries++) {
                    // the QP stage never shifts: ZZ may still hold the obstacle positions there (SRB_OBS_IN_ZZ)
                    LCK(nl || delta == 0.0, 7);
                    gj_load<NZL, NZE>(Mi, H0, ZZ, delta, nz, lane);    // H0 + delta Z'Z (the solves shift on the fly too)
                    // KF instances: the inverse in fp32 while mu > kkt32_mu (then nref fp64 refinement steps per solve)
                    int cf = (KF && f32) ? gj_invert_f32<NZL>(Mi, mrow<NZL>(lane), !nl) : gj_factor<NZL, NZE>(Mi, nz, lane, !nl);
#ifdef SRB_DIAG_FORCE_SHIFT        // diagnostic builds only: every NLP iteration's first factorisation counts as failed,
#ifndef SRB_DIAG_BUILD             // so the shift path runs on any batch (the suite reaches it with a raised Sw: tests/shift_cases.py)
#error "SRB_DIAG_FORCE_SHIFT is a diagnostic-build option"
#endif
                    if (nl && tries == 0) cf = 1;
#endif
                    if (cf == 0) { ok = 1; break; }
                    if (tries + 1 == ntries) break;             // no factorisation follows: no shift to form
                    if (delta == 0.0) {
                        // scale-aware first shift: 1e-10 * max(1, max diag of Z'HZ), formed only here, at the first
                        // failure (a wave reduction; the branch is uniform: cf comes from broadcast pivots, and with
                        // NW > 1 every wave factors the same H0, which nothing has written since the Gram)
                        const double dm = (lane < nz) ? H0[lane * LDH + lane] : 1.0;
                        delta = 1e-10 * fmax(1.0, wmax(dm));
                    } else {
                        delta *= 10.0;
                    }
                }
                STAMP_END(5);
                if (!ok) { flag = 1; break; }
                if (near && delta != 0.0) { flag = 4; break; }
            }

            // ---- predictor (pc) or centring step (Prime.c:193-196), then corrector
            double ap = 1.0, ad = 1.0;
#pragma clang loop unroll(disable)
            for (int pass = (pc ? 0 : 1); pass < 2; pass++) {
                if (pass == 1 || !pc) {
                    if constexpr (RSLS) {
                        set_rhs(1);                           // (pass is 1 here: without a predictor the loop starts at 1)
                        STAMP_END(6 + 4 * pass);
                        double cfr[TS];
                        int rr[TS];
#pragma unroll
                        for (int t = 0; t < TS; t++) { cfr[t] = Q[t].jd; rr[t] = Q[t].r; }
                        rhs_slots<NZL, NZE, TS>(R, cfr, rr, nts, vg, nz, lane);
                    } else {
                        set_rhs(pass);
                        SYNC();
                        STAMP_END(6 + 4 * pass);
                        rhs_only<NZL, NW>(R, CF, cnt, OF, nko, vg, nz, tid, part, bmask);
                    }
                    SYNC();
                    STAMP_END(7 + 4 * pass);
                }
                la_solve<NZL, NW, NZE, KF>(Mi, H0, ZZ, delta, vg, vy, vr, vd, dxi, nz, lane, (KF && f32) ? prm.kkt32_ref : SRB_REFINE);
                STAMP_END(8 + 4 * pass);
                // J dx per slot; dz = om (J dx - r3); ds = (dsT - s dz) / z; step-length maxima
                double mxs = 0.0, mxz = 0.0;
                // folded instances (N = 20): dx = Z dxi of every variable once (dxv; ceil(n / NTH) row dots a
                // lane instead of one per slot), then each slot's J dx from it: VAR / VEL dx_v, CoM-CoP
                // dx_p - dx_u, obstacle rows jx dx_px + jy dx_py - dx_s (config 5 1.81 -> 1.80 ms).  The
                // stored-row instances dot each slot's own row inside the slot loop (the separate pass measured
                // slower there: configs[2] 0.327 -> 0.340 ms)
                if constexpr (!SRB_OBS_STORED(NZL)) {
                    for (int v = tid; v < n; v += NTH) dxv[v] = row_dot<NZL, NZE>(R + TL.zr(v) * LDR, dxi);
                    SYNC();
                }
                // stored-row instances: two row buffers, slot t + 1's term row loaded before slot t's arithmetic,
                // so a pass waits for one LDS round trip, not one a slot
                double rw[SRB_OBS_STORED(NZL) ? 2 : 1][NZE];
                if constexpr (SRB_OBS_STORED(NZL))
                    if (0 < nts) row_load<NZE>(R + Q[0].r * LDR, rw[0]);
#pragma unroll
                for (int t = 0; t < TS; t++)
                    if (t < nts) {
                        Slot &q = Q[t];
                        const int kd = SK_KIND(q, t);
                        if constexpr (SRB_OBS_STORED(NZL)) {
                            LCK(q.r >= 0 && q.r < RROWS, 1);
                            if (t + 1 < TS && t + 1 < nts) row_load<NZE>(R + Q[(t + 1) % TS].r * LDR, rw[(t + 1) & 1]);
                            __builtin_amdgcn_sched_barrier(0);
                            q.jd = row_sum<NZL, NZE>(rw[t & 1], dxi);
                        } else if (SK_EQ(t, kd, K_OBS)) {            /* (QP stage: masked rows, 0) */
                            const int o = q.r - rO;
                            q.jd = nl ? fma(OJ[2 * o], dxv[q.i0], fma(OJ[2 * o + 1], dxv[q.i1], -dxv[n - 1])) : 0.0;
                        } else {
                            q.jd = SK_EQ(t, kd, K_COP) ? dxv[q.i0] - dxv[q.i1] : dxv[q.i0];
                        }
#pragma unroll
                        for (int r = 0; r < 2; r++)
                        if (SK_TWO(t) || r == 0) {
                            const double izr = IZ(q, r), isr = IS(q, r);
                            double dsT, r3;
                            if constexpr (LEAN) {                    // set_rhs(pass)'s terms, recomputed
                                dsT = -q.s[r] * q.z[r];
                                if (pass == 1 && pc) dsT -= q.ds[r] * q.dz[r];
                                dsT += (pass == 0) ? 0.0 : (pc ? sigma * mu : sigma_d * mu);
                                const double rz = r ? (q.h[1] - q.s[1] + fv[t]) : (q.h[0] - q.s[0] - fv[t]);
                                r3 = fma(-dsT, izr, rz);
                            } else {
                                dsT = q.dsT[r]; r3 = q.r3[r];
                            }
                            q.dz[r] = SK_M(q, t, r) * q.z[r] * isr * fma(r ? -1.0 : 1.0, q.jd, -r3);
                            q.ds[r] = SK_M(q, t, r) * fma(-q.s[r], q.dz[r], dsT) * izr;
                            mxs = fmax(mxs, -q.ds[r] * isr); mxz = fmax(mxz, -q.dz[r] * izr);
                        }
                    }
                STAMP_END(21 + pass);
                // findsteplength (Auxilary.c:271-294): 1 / max(-dv / v), 1 when no dv < 0
                {
                    double rv[2] = {mxs, mxz};
                    wred_x<2, 3u, NW>(rv, red + (3 + 2 * pass) * 8 * NW, tid);
                    mxs = rv[0]; mxz = rv[1];
                }
                ap = (mxs > 0.0) ? 1.0 / mxs : 1.0;
                ad = (mxz > 0.0) ? 1.0 / mxz : 1.0;
                STAMP_END(9 + 4 * pass);
                if (pass == 0) {
                    // rho = (s + ap ds)'(z + ad dz) / s'z ; sigma = min(1, rho)^3  (formrho, Prime.c:160-170)
                    double num = 0.0;
#pragma unroll
                    for (int t = 0; t < TS; t++)
                        if (t < nts) {
                            const Slot &q = Q[t];
                            num = fma(SK_M(q, t, 0) * fma(ap, q.ds[0], q.s[0]), fma(ad, q.dz[0], q.z[0]), num);
                            if (SK_TWO(t)) num = fma(SK_M(q, t, 1) * fma(ap, q.ds[1], q.s[1]), fma(ad, q.dz[1], q.z[1]), num);
                        }
                    {
                        double rv[1] = {num};
                        wred_x<1, 0u, NW>(rv, red + 4 * 8 * NW, tid);
                        num = rv[0];
                    }
                    const double rho = num / sz, mr = rho < 1.0 ? rho : 1.0;
                    sigma = mr * mr * mr; if (sigma < sigma_d) sigma = sigma_d;
                    continue;
                }
                if (near && (ap < SRB_NLP_BLOCKED || ad < SRB_NLP_BLOCKED)) { acc = true; break; }
                // ---- update (Prime.c:208-216): step 0.99 alpha capped at 1
                ap = (0.99 * ap < 1.0) ? 0.99 * ap : 1.0;
                ad = (0.99 * ad < 1.0) ? 0.99 * ad : 1.0;
                dxl = 0.0;
                NLPDBG(iter, 4, ap); NLPDBG(iter, 5, ad); NLPDBG(iter, 6, delta); NLPDBG(iter, 7, sigma);
                // rx' = (1-ad) rx + (ad-ap) P dx + ad (hess + delta) dx - (J(x') - J(x))' z'
                // (hess from the old obstacle duals in zo, the Jacobian change from the new ones)
                double hso[TS];
#pragma unroll
                for (int t = 0; t < TS; t++) {
                    hso[t] = 0.0;
                    if (t < nts) {
                        Slot &q = Q[t];
                        if (nl && SK_COM(t) && SK_IS(q, t, K_VAR) && q.i0 < 4 * N && !(q.i0 & 1)) {
                            const int k = q.i0 >> 2;
                            if constexpr (TK::compiled) hso[t] = hsc[t];     // zo is as the weights phase read it
                            else hso[t] = zo_sum(zo, k, K);
                        }
#pragma unroll
                        for (int r = 0; r < 2; r++)
                            if (SK_TWO(t) || r == 0) { q.s[r] = fma(ap, q.ds[r], q.s[r]); q.z[r] = fma(ad, q.dz[r], q.z[r]); }
                    }
                }
                SYNC();          // every lane has read the old duals and x
                STAMP_END(19);
#pragma unroll
                for (int t = 0; t < TS; t++)
                    if (t < nts) {
                        Slot &q = Q[t];
                        if (nl && SK_IS(q, t, K_OBS)) zo[q.r - rO] = q.z[0];
                        if (SK_IS(q, t, K_VAR)) {
                            dxl = fmax(dxl, fabs(ap * q.jd));
                            q.rx = (1.0 - ad) * q.rx + ((ad - ap) * q.a0) * q.jd;
                            if (nl) q.rx = fma(ad * (delta - 2.0 * hso[t]), q.jd, q.rx);
                            xprev[q.i0] = fv[t];                 // the iterate a non-finite step falls back to
                            xs[q.i0] = fma(ap, q.jd, fv[t]);
                        }
                    }
                SYNC();
                STAMP_END(20);
                if (nl)
#pragma unroll
                    for (int t = 0; t < TS; t++)
                        if (t < nts) {
                            Slot &q = Q[t];
                            if (SK_COM(t) && SK_IS(q, t, K_VAR) && q.i0 < 4 * N && !(q.i0 & 1)) {   // +2 ap dx sum_j z'_kj on (x_k, y_k)
                                const int k = q.i0 >> 2;
                                double hs_new = 0.0;
                                hs_new = zo_sum(zo, k, K);
                                if constexpr (TK::compiled) hsc[t] = hs_new;    // the next iteration's sum
                                q.rx = fma(2.0 * ap * hs_new, q.jd, q.rx);
                            }
                        }
                STAMP_END(14);
            }
            if (acc) { flag = 4; break; }
            it++;
        }
        if (flag == 0 && prov) flag = 4;
        if (nl && saved && !prov && (restore || flag == 2 || flag == 4)) {      // ACCEPTABLE / MAXIT: the best saved iterate
            for (int v = tid; v < n; v += NTH) xs[v] = xsv[v];     // owner threads, as saved
            flag = 4;                                               // (zpol_g: exported at the save)
        } else if ((zpol_g || prm.polish_fused) && nl) {
            export_zpol();
        }
        // a QP stage that stopped at the warm-start tolerance reports 4 (its point is the NLP's warm start, not
        // iSWIFT's 1e-6 point), never OPTIMAL (oracle/batch.c, the same rule)
        if (stage == 0) { qp_flag = (flag == 0 && tolS > tol) ? 4 : flag; qp_it = it; } else { nlp_flag = flag; nlp_it = it; }
