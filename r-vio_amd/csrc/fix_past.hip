// fix_past.hip — past-frame fixes (rvio_hip_update_fix_past[_dev] of include/rvio_hip.h): a world-frame position, attitude or pose that belongs to
// an image the filter consumed `age` frames ago, linearised against the pose the state still holds for that frame and handed to aux_update_kernel
// (aux_update.hip, unchanged) as a RESIDUAL-mode measurement, like fix_rows.hip does for a fix of now.  Stochastic cloning: the clone window IS the
// chain of relative poses between consecutive images, so the world pose of the IMU at any of the last n images is a function of (qG, pG) and the
// newest clones.
//
// Clone i (oldest first, x[26 + 7 i ..]) holds (q_i, p_i): C_i = R(q_i) rotates the older of two consecutive image frames into the newer, p_i is the
// newer frame's origin in the older (System.cc:279-321).  Behind augment / compose the newest clone ends at the reference frame {R}.  With
// R_G = R(qG), l = lever and the age a = 0 .. n counted in images back from {R} (a = 0: {R} itself; the current (qk, pk) does not enter):
//   A_0 = I, t_0 = 0;   A_m = A_{m-1} C_{n-m},   t_m = t_{m-1} - A_m p_{n-m}      (m = 1 .. a)
//   u_a = t_a + A_a l,  s_a = u_a - pG
//   POSITION  h_a = R_G^T s_a               r = z[0:3] - h_a
//             cols 0-2: -R_G^T [s_a x]   3-5: -R_G^T   clone n - m:  rotation R_G^T [(u_a - t_{m-1}) x] A_{m-1}   position -R_G^T A_m
//   ATTITUDE  R(world -> IMU then) = A_a^T R_G;  E = R(z[3:7])^T A_a^T R_G,  r = (E21 - E12, E02 - E20, E10 - E01) / 2
//             cols 0-2: R_G^T                          clone n - m:  rotation -R_G^T A_{m-1}
//   POSE      the three position rows, then the three attitude rows
// POSITION with frac = lam in (0, 1): the stamp lies lam of the way from the frame a back towards the frame a + 1 back; h and every block are
// (1 - lam) x those of a + lam x those of a + 1.  Every column not listed — 6 .. 23 and every clone older than the ones the chain passes — is 0.0.
//
// One launch, gridDim.z = instances, ONE wave per instance (LP_FIXP_T = 64), FP64, plain C++.  The chain is a product of at most LP_FIXP_NMAX rigid
// transforms (A, t) o (C, -C p) = (A C, t - A C p), which is associative: lane m - 1 forms the element of clone n - m, an inclusive scan over the
// wave (log2 steps of __shfl_up, a 3 x 3 product each) leaves (A_m, t_m) in lane m - 1, and every lane drops its pair into static LDS so that all
// of them can read A_{m-1}, t_{m-1}, A_a, t_a.  Lane 0 places the head blocks in the cleared 6 x 24 head (as fix_rows_kernel does) and writes r,
// sigma, the record and the cleared (gamma, applied) pair; then the wave stores the head columns from LDS and lane m - 1 the 6 columns of clone
// n - m in all rows (0.0 where the chain does not reach) — every element of the rows is written once, by one lane.  No atomics, no dynamic LDS.
//
// The kernel owns an active flag per instance: the caller's flag AND age / frac inside the window.  aux_update_kernel gets THAT flag, so an
// instance whose age is outside 0 .. n (or a + 1 > n with lam > 0, lam outside [0, 1), lam > 0 with a kind other than POSITION) is written by
// neither launch; its record says so: m = 0, applied = 0, img_count = -1, r = 0.  An instance the caller flagged inactive gets flag 0 and nothing else.

struct fixp_rt { m33 A; d3 t; };
__device__ __forceinline__ fixp_rt fixp_ld(const double* chain, int m) {
    fixp_rt e;
    const double* c = chain + 12 * m;
#pragma unroll
    for (int k = 0; k < 9; ++k) e.A.m[k] = c[k];
    e.t = mk3(c[9], c[10], c[11]);
    return e;
}
__device__ __forceinline__ m33 fixp_mix(double wa, const m33& Xa, double wb, const m33& Xb) {
    m33 C;
#pragma unroll
    for (int k = 0; k < 9; ++k) C.m[k] = wa * Xa.m[k] + wb * Xb.m[k];
    return C;
}

// x: instance 0's state, instance z lies bs bytes behind; fix: instance 0's, fix_bs BYTES between instances (0: shared); age: one per instance;
// frac: NULL (0) or one per instance; active: NULL or one flag per instance; ref_count: the frame count of {R}; H: instance 0's rows, H_bs bytes
// between instances; r / sigma: 6 per instance; rec / pair / flag: one per instance; n: clones now (<= LP_FIXP_NMAX)
__global__ __launch_bounds__(LP_FIXP_T) void fix_past_kernel(int n, int kind, const double* x, size_t bs, const rvio_fix* fix, size_t fix_bs, const int* age,
                                                            const double* frac, const int* active, int ref_count, double* H, size_t H_bs, double* r,
                                                            double* sigma, rvio_fix_diag* rec, double* pair, int* flag) {
    static_assert(LP_FIXP_T == 64, "one wave per instance");
    __shared__ double head[LP_FIX_HEAD];
    __shared__ double chain[LP_FIXP_CHAIN];
    const int z = (int)blockIdx.z, lane = (int)threadIdx.x;
    if (active && active[z] == 0) { if (lane == 0) flag[z] = 0; return; }
    const int a = age[z];
    const double lam = frac ? frac[z] : 0.0;
    const bool interp = lam > 0.0;
    const int amax = a + (interp ? 1 : 0);
    const bool pos = kind == RVIO_FIX_POSITION || kind == RVIO_FIX_POSE, att = kind == RVIO_FIX_ATTITUDE || kind == RVIO_FIX_POSE;
    const bool ok = n <= LP_FIXP_NMAX && a >= 0 && amax <= n && lam >= 0.0 && lam < 1.0 && (!interp || kind == RVIO_FIX_POSITION);
    if (!ok) {
        if (lane == 0) {
            rvio_fix_diag* out = rec + z;
#pragma unroll
            for (int i = 0; i < 6; ++i) { r[6 * (size_t)z + i] = 0.0; out->r[i] = 0.0; }
            out->gamma = 0.0; out->applied = 0; out->kind = kind; out->m = 0; out->img_count = -1;
            pair[2 * (size_t)z] = 0.0; ((long long*)pair)[2 * (size_t)z + 1] = 0;
            flag[z] = 0;
        }
        return;
    }
    x = zoffi(x, bs, z);
    fix = zoffi(fix, fix_bs, z);
    H = zoffi(H, H_bs, z);
    const int m = kind == RVIO_FIX_POSE ? 6 : 3, d = 24 + 6 * n;
    for (int e = lane; e < LP_FIX_HEAD; e += LP_FIXP_T) head[e] = 0.0;

    // ---- the chain: lane m - 1 holds the element of clone n - m, the identity where the chain does not reach
    const int mm = lane + 1;
    fixp_rt e;
    e.A = eye33(); e.t = mk3(0.0, 0.0, 0.0);
    if (mm <= amax) {
        const double* c = x + 26 + 7 * (n - mm);
        e.A = q2r(ldq(c));
        e.t = scl3(-1.0, mv33(e.A, ld3(c + 4)));
    }
    for (int off = 1; off < amax; off <<= 1) {          // (uniform: amax is the instance's)
        fixp_rt o;
#pragma unroll
        for (int k = 0; k < 9; ++k) o.A.m[k] = __shfl_up(e.A.m[k], off, LP_FIXP_T);
        o.t.x = __shfl_up(e.t.x, off, LP_FIXP_T); o.t.y = __shfl_up(e.t.y, off, LP_FIXP_T); o.t.z = __shfl_up(e.t.z, off, LP_FIXP_T);
        if (lane >= off) { e.t = add3(o.t, mv33(o.A, e.t)); e.A = mul33(o.A, e.A); }
    }
    if (mm <= amax) {
        double* c = chain + 12 * mm;
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] = e.A.m[k];
        c[9] = e.t.x; c[10] = e.t.y; c[11] = e.t.z;
    }
    if (lane == LP_FIXP_T - 1) {
#pragma unroll
        for (int k = 0; k < 12; ++k) chain[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    }
    __syncthreads();

    // ---- head, residual, record (every lane forms them, lane 0 stores)
    const m33 RG = q2r(ldq(x));
    const m33 RGt = tr33(RG);
    const d3 pG = ld3(x + 4);
    const d3 l = pos ? ld3(fix->lever) : mk3(0.0, 0.0, 0.0);
    const fixp_rt Ea = fixp_ld(chain, a);
    const d3 ua = add3(Ea.t, mv33(Ea.A, l));
    d3 ub = ua;
    if (interp) { const fixp_rt Eb = fixp_ld(chain, a + 1); ub = add3(Eb.t, mv33(Eb.A, l)); }
    const double wa = interp ? 1.0 - lam : 1.0, wb = interp ? lam : 0.0;
    if (lane == 0) {
        double res[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (pos) {
            const d3 sa = sub3(ua, pG);
            d3 hp = mv33(RGt, sa);
            m33 B0 = scl33(-1.0, mul33(RGt, skew33(sa))), B1 = scl33(-1.0, RGt);
            if (interp) {
                const d3 sb = sub3(ub, pG), hb = mv33(RGt, sb);
                hp = add3(scl3(wa, hp), scl3(wb, hb));
                B0 = fixp_mix(wa, B0, wb, scl33(-1.0, mul33(RGt, skew33(sb))));
                B1 = fixp_mix(wa, B1, wb, B1);
            }
            fix_put33(head, 0, 0, B0); fix_put33(head, 0, 3, B1);
            res[0] = fix->z[0] - hp.x; res[1] = fix->z[1] - hp.y; res[2] = fix->z[2] - hp.z;
            sg[0] = fix->sigma[0]; sg[1] = fix->sigma[1]; sg[2] = fix->sigma[2];
        }
        if (att) {
            const int o = pos ? 3 : 0;
            const m33 E = mul33(mul33(tr33(q2r(ldq(fix->z + 3))), tr33(Ea.A)), RG);
            fix_put33(head, o, 0, RGt);
            res[o] = 0.5 * (E.m[7] - E.m[5]); res[o + 1] = 0.5 * (E.m[2] - E.m[6]); res[o + 2] = 0.5 * (E.m[3] - E.m[1]);
            sg[o] = fix->sigma[3]; sg[o + 1] = fix->sigma[4]; sg[o + 2] = fix->sigma[5];
        }
        double* rz = r + 6 * (size_t)z;
        double* sz = sigma + 6 * (size_t)z;
        rvio_fix_diag* out = rec + z;
#pragma unroll
        for (int i = 0; i < 6; ++i) { rz[i] = res[i]; sz[i] = sg[i]; out->r[i] = res[i]; }
        out->gamma = 0.0; out->applied = 0; out->kind = kind; out->m = m; out->img_count = ref_count - a;
        pair[2 * (size_t)z] = 0.0; ((long long*)pair)[2 * (size_t)z + 1] = 0;
        flag[z] = 1;
    }
    __syncthreads();

    // ---- the rows: head columns from LDS, then lane m - 1 the six columns of clone n - m
    for (int k = lane; k < m * 24; k += LP_FIXP_T) {
        const int row = k / 24, col = k - row * 24;
        H[row * d + col] = head[k];
    }
    if (mm <= n) {
        m33 Pr, Pp, Ar;
#pragma unroll
        for (int k = 0; k < 9; ++k) { Pr.m[k] = 0.0; Pp.m[k] = 0.0; Ar.m[k] = 0.0; }
        if (mm <= amax) {
            const fixp_rt E0 = fixp_ld(chain, mm - 1), E1 = fixp_ld(chain, mm);
            if (pos) {
                const m33 Xp = scl33(-1.0, mul33(RGt, E1.A));
                const m33 Xb = mul33(mul33(RGt, skew33(sub3(ub, E0.t))), E0.A);
                if (mm <= a) {
                    const m33 Xa = mul33(mul33(RGt, skew33(sub3(ua, E0.t))), E0.A);
                    Pr = interp ? fixp_mix(wa, Xa, wb, Xb) : Xa;
                    Pp = interp ? fixp_mix(wa, Xp, wb, Xp) : Xp;
                } else {
                    Pr = scl33(wb, Xb);
                    Pp = scl33(wb, Xp);
                }
            }
            if (att && mm <= a) Ar = scl33(-1.0, mul33(RGt, E0.A));
        }
        double* Hc = H + 24 + 6 * (n - mm);
        if (pos) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) { Hc[i * d + j] = Pr.m[3 * i + j]; Hc[i * d + 3 + j] = Pp.m[3 * i + j]; }
        }
        if (att) {
            const int o = pos ? 3 : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) { Hc[(o + i) * d + j] = Ar.m[3 * i + j]; Hc[(o + i) * d + 3 + j] = 0.0; }
        }
    }
}
