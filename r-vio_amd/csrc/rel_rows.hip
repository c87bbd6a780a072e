// rel_rows.hip — relative-pose measurements (rvio_hip_update_rel[_dev] of include/rvio_hip.h): the delta pose between two frames of the clone
// window — what a wheel-odometry integrator, a scan matcher, a second visual odometry or a loop closure inside the window produces — linearised
// against the clones between the two frames and handed to aux_update_kernel (aux_update.hip, unchanged) as a RESIDUAL-mode measurement, like
// fix_rows.hip and fix_past.hip do for world-frame fixes.  The robocentric window IS the chain of relative poses between consecutive images, so
// the pose of the frame a images back in the frame b > a images back depends on the clones n - b .. n - a - 1 and on nothing else: not on
// (qG, pG), (qk, pk), velocity or biases, not on any newer or older clone.
//
// Clone i (oldest first, x[26 + 7 i ..]) holds (q_i, p_i): C_i = R(q_i) rotates the older of two consecutive image frames into the newer, p_i is the
// newer frame's origin in the older.  Ages count images back from the reference frame {R} as in fix_past.hip; a = age_new, b = age_old,
// 0 <= a < b <= n, k = b - a, l = lever, i_j = n - a - j:
//   B_0 = I, s_0 = 0;   B_j = B_{j-1} C_{i_j},   s_j = s_{j-1} - B_j p_{i_j}      (j = 1 .. k)
//   REL_POSITION  h = B_k^T (l - s_k) - l          r = z[0:3] - h
//                 clone i_j:  rotation -B_k^T [(l - s_{j-1}) x] B_{j-1}   position B_k^T B_j
//   REL_ATTITUDE  E = B_k R(z[3:7])^T,  r = (E21 - E12, E02 - E20, E10 - E01) / 2
//                 clone i_j:  rotation B_{j-1}                             position 0
//   REL_POSE      the three position rows, then the three attitude rows
// Every column not listed — all of 0 .. 23 and every clone outside n - b .. n - a - 1 — is 0.0.
//
// One launch, gridDim.z = instances, ONE wave per instance (LP_FIXP_T = 64), FP64, plain C++: the launch form of fix_past_kernel, whose rigid
// element (fixp_rt), chain layout (LP_FIXP_CHAIN, fixp_ld) and matrix helpers it uses as they are.  Lane mm - 1 owns clone n - mm and forms its
// element (C, -C p) when a < mm <= b, the identity otherwise; an inclusive scan over the wave (log2 steps of __shfl_up, bounded by the instance's
// own b) leaves (B_{mm-a}, s_{mm-a}) in lane mm - 1, and every lane of the span drops its pair into static LDS so that all of them can read
// B_{j-1}, s_{j-1}, B_k.  Lane 0 writes r, sigma, the record and the cleared (gamma, applied) pair; the wave stores zeros to the 24 head columns
// and lane mm - 1 the six columns of clone n - mm in all rows (0.0 where the span does not reach) — every element of the rows is written once, by
// one lane.  No atomics, no dynamic LDS, no head block (the head is all zero).
//
// The kernel owns an active flag per instance: the caller's flag AND 0 <= a < b <= n.  aux_update_kernel gets THAT flag, so an instance whose span
// is outside the window is written by neither launch; its record says so: m = 0, applied = 0, img_count = -1, r = 0.  An instance the caller
// flagged inactive gets flag 0 and nothing else.

// x: instance 0's state, instance z lies bs bytes behind; meas: instance 0's, meas_bs BYTES between instances (0: shared); age_new / age_old: one
// per instance; active: NULL or one flag per instance; ref_count: the frame count of {R}; H: instance 0's rows, H_bs bytes between instances;
// r / sigma: 6 per instance; rec / pair / flag: one per instance; n: clones now (<= LP_FIXP_NMAX); kind: RVIO_REL_*
__global__ __launch_bounds__(LP_FIXP_T) void rel_rows_kernel(int n, int kind, const double* x, size_t bs, const rvio_fix* meas, size_t meas_bs, const int* age_new,
                                                            const int* age_old, const int* active, int ref_count, double* H, size_t H_bs, double* r, double* sigma,
                                                            rvio_fix_diag* rec, double* pair, int* flag) {
    static_assert(LP_FIXP_T == 64 && LP_FIXP_NMAX < LP_FIXP_T, "one wave per instance, one lane per clone");
    __shared__ double chain[LP_FIXP_CHAIN];
    const int z = (int)blockIdx.z, lane = (int)threadIdx.x;
    if (active && active[z] == 0) { if (lane == 0) flag[z] = 0; return; }
    const int a = age_new[z], b = age_old[z];
    const bool pos = kind == RVIO_REL_POSITION || kind == RVIO_REL_POSE, att = kind == RVIO_REL_ATTITUDE || kind == RVIO_REL_POSE;
    const bool ok = n <= LP_FIXP_NMAX && a >= 0 && a < b && b <= n;
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
    meas = zoffi(meas, meas_bs, z);
    H = zoffi(H, H_bs, z);
    const int m = kind == RVIO_REL_POSE ? 6 : 3, d = 24 + 6 * n, k = b - a;

    // ---- the chain: lane mm - 1 holds the element of clone n - mm inside the span, the identity outside it
    const int mm = lane + 1;
    const bool in_span = mm > a && mm <= b;
    fixp_rt e;
    e.A = eye33(); e.t = mk3(0.0, 0.0, 0.0);
    if (in_span) {
        const double* c = x + 26 + 7 * (n - mm);
        e.A = q2r(ldq(c));
        e.t = scl3(-1.0, mv33(e.A, ld3(c + 4)));
    }
    for (int off = 1; off < b; off <<= 1) {          // (uniform: b is the instance's)
        fixp_rt o;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.A.m[i] = __shfl_up(e.A.m[i], off, LP_FIXP_T);
        o.t.x = __shfl_up(e.t.x, off, LP_FIXP_T); o.t.y = __shfl_up(e.t.y, off, LP_FIXP_T); o.t.z = __shfl_up(e.t.z, off, LP_FIXP_T);
        if (lane >= off) { e.t = add3(o.t, mv33(o.A, e.t)); e.A = mul33(o.A, e.A); }
    }
    if (in_span) {                                   // (B_j, s_j) at chain[12 j], j = mm - a = 1 .. k <= LP_FIXP_NMAX
        double* c = chain + 12 * (mm - a);
#pragma unroll
        for (int i = 0; i < 9; ++i) c[i] = e.A.m[i];
        c[9] = e.t.x; c[10] = e.t.y; c[11] = e.t.z;
    }
    if (lane == LP_FIXP_T - 1) {
#pragma unroll
        for (int i = 0; i < 12; ++i) chain[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    }
    __syncthreads();

    // ---- residual, record (lane 0)
    const d3 l = pos ? ld3(meas->lever) : mk3(0.0, 0.0, 0.0);
    const fixp_rt Ek = fixp_ld(chain, k);
    const m33 Bkt = tr33(Ek.A);
    if (lane == 0) {
        double res[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (pos) {
            const d3 hp = sub3(mv33(Bkt, sub3(l, Ek.t)), l);
            res[0] = meas->z[0] - hp.x; res[1] = meas->z[1] - hp.y; res[2] = meas->z[2] - hp.z;
            sg[0] = meas->sigma[0]; sg[1] = meas->sigma[1]; sg[2] = meas->sigma[2];
        }
        if (att) {
            const int o = pos ? 3 : 0;
            const m33 E = mul33(Ek.A, tr33(q2r(ldq(meas->z + 3))));
            res[o] = 0.5 * (E.m[7] - E.m[5]); res[o + 1] = 0.5 * (E.m[2] - E.m[6]); res[o + 2] = 0.5 * (E.m[3] - E.m[1]);
            sg[o] = meas->sigma[3]; sg[o + 1] = meas->sigma[4]; sg[o + 2] = meas->sigma[5];
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

    // ---- the rows: zeros in the head columns, then lane mm - 1 the six columns of clone n - mm
    for (int e24 = lane; e24 < m * 24; e24 += LP_FIXP_T) {
        const int row = e24 / 24, col = e24 - row * 24;
        H[row * d + col] = 0.0;
    }
    if (mm <= n) {
        m33 Pr, Pp, Ar;
#pragma unroll
        for (int i = 0; i < 9; ++i) { Pr.m[i] = 0.0; Pp.m[i] = 0.0; Ar.m[i] = 0.0; }
        if (in_span) {
            const fixp_rt E0 = fixp_ld(chain, mm - a - 1), E1 = fixp_ld(chain, mm - a);
            if (pos) {
                Pr = scl33(-1.0, mul33(mul33(Bkt, skew33(sub3(l, E0.t))), E0.A));
                Pp = mul33(Bkt, E1.A);
            }
            if (att) Ar = E0.A;
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
