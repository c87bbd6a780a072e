// fix_rows.hip — absolute fixes (rvio_hip_update_fix[_dev] of include/rvio_hip.h): a world-frame position, attitude or pose, or the accelerometer
// at rest, linearised AT THE INSTANCE'S CURRENT STATE, where that state lies, and handed to aux_update_kernel (aux_update.hip, unchanged) as a
// RESIDUAL-mode measurement: H (m x d, row-major), r, sigma.  A second producer in front of the same consumer, beside standstill_kernel.
//
// The state is robocentric, x = qG pG g qk pk v bg ba | clones; the error convention of every rotation slot is R_true ~ (I - [dth x]) R
// (Updater.cc:549-563).  With R_G = R(qG), R_k = R(qk) (an all-zero qk reads as I, as QuatToRot gives it), R = R_k R_G, l = lever,
// s = pk - pG + R_k^T l, G = cfg.gravity, columns as in P:
//   POSITION  h = R_G^T s                 r = z[0:3] - h      cols 0-2: -R_G^T [s x]   3-5: -R_G^T   9-11: -R_G^T R_k^T [l x]   12-14: R_G^T
//   ATTITUDE  world-frame rotation error  E = R(z[3:7])^T R,  r = (E21 - E12, E02 - E20, E10 - E01) / 2
//             of R_wb = R^T                                   cols 0-2: R_G^T          9-11: R^T
//   POSE      the three position rows, then the three attitude rows
//   GRAVITY   h = ba + G R_k g            r = z[0:3] - h      cols 6-8: G R_k          9-11: G [R_k g x]     21-23: I
//             (PreIntegrator.cc:107, 175-177 at rest)
// Every other column, the clone columns among them, is exactly 0.0.
//
// One launch, gridDim.z = instances, ONE wave per instance (LP_FIX_T = 64).  Every lane forms the same 3 x 3 products in registers (FP64, plain
// C++; a dozen dependent products: the kernel is bound by latency, not by anything a wider workgroup would hide), lane 0 places the blocks in
// the 6 x 24 head held in static LDS, which the wave has cleared, and the wave then stores the m x d rows for the window as it is now: head
// columns from LDS, clone columns 0.0 — every element of the rows is written once, by one lane.  Lane 0 also stores r, sigma, the record
// (r, kind, m, img_count) and clears the (gamma, applied) pair that aux_update_kernel rewrites when it runs.  No atomics, no dynamic LDS.
// An inactive instance (active[z] == 0) is skipped: nothing of it is written here, and the aux launch behind gets the same flags.
// Only x[0:26] of the instance and its rvio_fix are read; what the kind does not use of the fix (a lever with ATTITUDE, a quaternion with
// POSITION) is not looked at.

__device__ __forceinline__ void fix_put33(double* head, int row0, int col0, const m33& A) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) head[(row0 + i) * 24 + col0 + j] = A.m[3 * i + j];
}

// x: instance 0's state, instance z lies bs bytes behind; fix: instance 0's, fix_bs BYTES between instances (0: shared); active: NULL or one flag
// per instance; H: instance 0's rows, H_bs bytes between instances; r / sigma: 6 per instance; rec / pair: one per instance; n: clones now
__global__ __launch_bounds__(LP_FIX_T) void fix_rows_kernel(int n, int kind, double G, const double* x, size_t bs, const rvio_fix* fix, size_t fix_bs,
                                                           const int* active, int img_count, double* H, size_t H_bs, double* r, double* sigma,
                                                           rvio_fix_diag* rec, double* pair) {
    static_assert(LP_FIX_T == 64, "one wave per instance");
    __shared__ double head[LP_FIX_HEAD];
    const int z = (int)blockIdx.z, lane = (int)threadIdx.x;
    if (active && active[z] == 0) return;
    x = zoffi(x, bs, z);
    fix = zoffi(fix, fix_bs, z);
    H = zoffi(H, H_bs, z);
    const bool pos = kind == RVIO_FIX_POSITION || kind == RVIO_FIX_POSE, att = kind == RVIO_FIX_ATTITUDE || kind == RVIO_FIX_POSE;
    const int m = kind == RVIO_FIX_POSE ? 6 : 3, d = 24 + 6 * n;
    for (int e = lane; e < LP_FIX_HEAD; e += LP_FIX_T) head[e] = 0.0;
    __syncthreads();
    const m33 RG = q2r(ldq(x)), Rk = q2r(ldq(x + 10));
    const m33 RGt = tr33(RG);
    double res[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    m33 B0, B1, B2, B3;          // the blocks of the position / gravity rows
    m33 A0, A1;                  // ... and of the attitude rows
    if (pos) {
        const d3 l = ld3(fix->lever);
        const m33 Rkt = tr33(Rk);
        const d3 s = add3(sub3(ld3(x + 14), ld3(x + 4)), mv33(Rkt, l));
        const d3 hp = mv33(RGt, s);
        B0 = scl33(-1.0, mul33(RGt, skew33(s)));
        B1 = scl33(-1.0, RGt);
        B2 = scl33(-1.0, mul33(mul33(RGt, Rkt), skew33(l)));
        B3 = RGt;
        res[0] = fix->z[0] - hp.x; res[1] = fix->z[1] - hp.y; res[2] = fix->z[2] - hp.z;
        sg[0] = fix->sigma[0]; sg[1] = fix->sigma[1]; sg[2] = fix->sigma[2];
    }
    if (att) {
        const int o = pos ? 3 : 0;
        const m33 R = mul33(Rk, RG);
        const m33 E = mul33(tr33(q2r(ldq(fix->z + 3))), R);
        A0 = RGt;
        A1 = tr33(R);
        res[o] = 0.5 * (E.m[7] - E.m[5]); res[o + 1] = 0.5 * (E.m[2] - E.m[6]); res[o + 2] = 0.5 * (E.m[3] - E.m[1]);
        sg[o] = fix->sigma[3]; sg[o + 1] = fix->sigma[4]; sg[o + 2] = fix->sigma[5];
    }
    if (kind == RVIO_FIX_GRAVITY) {
        const d3 gk = mv33(Rk, ld3(x + 7));
        B0 = scl33(G, Rk);
        B1 = scl33(G, skew33(gk));
        B2 = eye33();
        res[0] = fix->z[0] - (x[23] + G * gk.x); res[1] = fix->z[1] - (x[24] + G * gk.y); res[2] = fix->z[2] - (x[25] + G * gk.z);
        sg[0] = fix->sigma[0]; sg[1] = fix->sigma[1]; sg[2] = fix->sigma[2];
    }
    if (lane == 0) {
        if (pos) { fix_put33(head, 0, 0, B0); fix_put33(head, 0, 3, B1); fix_put33(head, 0, 9, B2); fix_put33(head, 0, 12, B3); }
        if (att) { const int o = pos ? 3 : 0; fix_put33(head, o, 0, A0); fix_put33(head, o, 9, A1); }
        if (kind == RVIO_FIX_GRAVITY) { fix_put33(head, 0, 6, B0); fix_put33(head, 0, 9, B1); fix_put33(head, 0, 21, B2); }
        double* rz = r + 6 * (size_t)z;
        double* sz = sigma + 6 * (size_t)z;
        rvio_fix_diag* out = rec + z;
#pragma unroll
        for (int i = 0; i < 6; ++i) { rz[i] = res[i]; sz[i] = sg[i]; out->r[i] = res[i]; }
        out->gamma = 0.0; out->applied = 0; out->kind = kind; out->m = m; out->img_count = img_count;
        pair[2 * (size_t)z] = 0.0; ((long long*)pair)[2 * (size_t)z + 1] = 0;
    }
    __syncthreads();
    for (int e = lane; e < m * d; e += LP_FIX_T) {
        const int row = e / d, col = e - row * d;
        H[e] = col < 24 ? head[row * 24 + col] : 0.0;
    }
}
