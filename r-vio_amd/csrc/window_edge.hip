// window_edge.hip — pose-graph export (rvio_window_edge, rvio_hip_get_window_edges*, rvio_hip_set_edge_odometry, rvio_hip_get_window_joint* of
// include/rvio_hip.h): what a pose-graph back end is fed from the clone window — BETWEEN-FACTORS, the relative pose of two frames with the covariance
// of that quantity, and the JOINT covariance of the world poses window_pose.hip publishes one by one.
//
// ---- window_edge_kernel.  Frames, ages and the local chain are those of rel_rows.hip: a = age_new, b = age_old, 0 <= a < b <= n, k = b - a,
// i_j = n - a - j:
//   B_0 = I, s_0 = 0;   B_j = B_{j-1} C_{i_j},   s_j = s_{j-1} - B_j p_{i_j}      (j = 1 .. k)
//   p    = -B_k^T s_k                              the origin of frame a in frame b, frame-b axes (rel_h's z[0:3] at lever 0)
//   R(q) = B_k                                     rotates frame b into frame a (the sense of a clone's q), RotToQuat's sign, q[3] >= 0
//   H    = the six RVIO_REL_POSE rows at lever 0 (6 x d), zero outside the clones n - b .. n - a - 1:
//     clone i_j:   rotation  B_k^T [s_{j-1} x] B_{j-1} | B_{j-1}      position  B_k^T B_j | 0
//   cov  = (C + C^T) / 2,  C = H P H^T             rows 0-2 along frame-b axes, rows 3-5 the rotation error along frame-a axes under
//                                                  R_true ~ (I - [dth x]) R: the order in which rvio_hip_update_rel(RVIO_REL_POSE) takes sigma
// The span of columns is contiguous: 24 + 6 (n - b) .. 24 + 6 (n - a) - 1, nz = 6 k <= LP_WEDGE_NZ of them; entry e <-> column c0 + e.
//
// Grid (pairs, 1, instances), ONE workgroup of LP_WEDGE_T = 256 threads per (instance, pair), FP64, plain C++, static LDS only, no atomics.
//   1  every wave forms the chain by the in-wave scan of rel_rows_kernel (lane mm - 1 <-> clone n - mm, an element inside the span, the
//      identity outside); wave 0 drops it into LDS
//   2  Hs[entry][row]: thread mm - 1 the six columns of clone n - mm; thread 64 forms p, q and the counts
//   3  T = P_span H^T: thread <-> entry, six accumulators, P read along columns (consecutive threads, consecutive doubles)
//   4  C = H T: window_pose_kernel's reduction — thread (g, entry (i, j)) forms its share of C_ij AND of C_ji over e = g, g + 7, ...; thread entry
//      adds the seven shares in the order 0 .. 6 and halves the sum of the two, so (i, j) and (j, i) carry the same bits, the same every run
//   5  the 47 words of the record from LDS: one coalesced store
// It reads the clones n - b .. n - a - 1 and the span's square of P; it writes its record, nothing else.
// A pair that is not 0 <= a < b <= n: img_count_new = -1, n_clones set, every other word 0.
__device__ __forceinline__ void wedge_put33(double* Hs, int e0, int row0, const m33& X) {   // block X at entries e0 .. e0 + 2, rows row0 .. row0 + 2
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Hs[(e0 + j) * 6 + row0 + i] = X.m[3 * i + j];
}

// x / P: instance 0's, instance z lies bs bytes behind; ld: leading dimension of P; n: clones now; the workgroup (b, 0, z) forms the record of the
// pair (age_new[b], age_old[b]) — one list for every instance; a NULL list: the pair (a0, b0) — into out[z * out_stride + b]; ref_count: the
// frame count of {R}
__global__ __launch_bounds__(LP_WEDGE_T) void window_edge_kernel(int n, int ld, const double* __restrict__ x, const double* __restrict__ P, size_t bs,
                                                                 const int* __restrict__ age_new, const int* __restrict__ age_old, int a0, int b0,
                                                                 int ref_count, long long seq, unsigned long long* __restrict__ out, size_t out_stride) {
    static_assert(LP_WEDGE_T == 256 && LP_FIXP_NMAX < 64 && LP_WEDGE_GROUPS * 36 <= LP_WEDGE_T && LP_WEDGE_WORDS <= LP_WEDGE_T, "four waves, one lane per clone");
    static_assert(LP_WEDGE_NZ >= 6 * LP_FIXP_NMAX, "room for the longest span the guard below lets through");
    __shared__ double chain[LP_FIXP_CHAIN];
    __shared__ __align__(16) double Hs[LP_WEDGE_NZ * 6];
    __shared__ __align__(16) double Ts[LP_WEDGE_NZ * 6];
    __shared__ double part[LP_WEDGE_GROUPS * 36 * 2];
    __shared__ unsigned long long rec[LP_WEDGE_WORDS];
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int a = age_new ? age_new[blockIdx.x] : a0, b = age_old ? age_old[blockIdx.x] : b0;
    out += (size_t)z * out_stride * LP_WEDGE_WORDS + (size_t)blockIdx.x * LP_WEDGE_WORDS;
    if (!(n >= 0 && n <= LP_FIXP_NMAX && a >= 0 && a < b && b <= n)) {
        if (tid < LP_WEDGE_WORDS) {
            unsigned long long w = 0ull;
            if (tid == 1) w = 0xffffffffull;                              // img_count_new = -1, img_count_old = 0
            if (tid == 3) w = (unsigned long long)(unsigned)n;            // n_clones, reserved = 0
            out[tid] = w;
        }
        return;
    }
    x = zoffi(x, bs, z);
    P = zoffi(P, bs, z);
    const int k = b - a;

    // ---- 1  the chain: lane mm - 1 holds the element of clone n - mm inside the span, the identity outside it
    {
        const int mm = lane + 1;
        const bool in_span = mm > a && mm <= b;
        fixp_rt e;
        e.A = eye33(); e.t = mk3(0.0, 0.0, 0.0);
        if (in_span) {
            const double* c = x + 26 + 7 * (n - mm);
            e.A = q2r(ldq(c));
            e.t = scl3(-1.0, mv33(e.A, ld3(c + 4)));
        }
        for (int off = 1; off < b; off <<= 1) {          // (uniform: b is the workgroup's)
            fixp_rt o;
#pragma unroll
            for (int i = 0; i < 9; ++i) o.A.m[i] = __shfl_up(e.A.m[i], off, 64);
            o.t.x = __shfl_up(e.t.x, off, 64); o.t.y = __shfl_up(e.t.y, off, 64); o.t.z = __shfl_up(e.t.z, off, 64);
            if (lane >= off) { e.t = add3(o.t, mv33(o.A, e.t)); e.A = mul33(o.A, e.A); }
        }
        if (wv == 0 && in_span) {                        // (B_j, s_j) at chain[12 j], j = mm - a = 1 .. k <= LP_FIXP_NMAX
            double* c = chain + 12 * (mm - a);
#pragma unroll
            for (int i = 0; i < 9; ++i) c[i] = e.A.m[i];
            c[9] = e.t.x; c[10] = e.t.y; c[11] = e.t.z;
        }
        if (tid == 63) {
#pragma unroll
            for (int i = 0; i < 12; ++i) chain[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        }
    }
    __syncthreads();

    // ---- 2  the columns of H that are not zero, Hs[entry * 6 + row]; thread 64 forms p, q and the counts
    const int nz = 6 * k, c0 = 24 + 6 * (n - b);
    {
        const int mm = tid + 1;
        const bool in_span = mm > a && mm <= b;
        if (in_span || tid == 64) {
            const d3 l = mk3(0.0, 0.0, 0.0);
            const fixp_rt Ek = fixp_ld(chain, k);
            const m33 Bkt = tr33(Ek.A);
            if (tid == 64) {
                const d3 p = sub3(mv33(Bkt, sub3(l, Ek.t)), l);
                const q4 q = r2q(Ek.A);
                rec[0] = (unsigned long long)seq;
                rec[1] = (unsigned long long)(unsigned)(ref_count - a) | ((unsigned long long)(unsigned)(ref_count - b) << 32);
                rec[2] = (unsigned long long)(unsigned)a | ((unsigned long long)(unsigned)b << 32);
                rec[3] = (unsigned long long)(unsigned)n;
                rec[4] = (unsigned long long)__double_as_longlong(p.x); rec[5] = (unsigned long long)__double_as_longlong(p.y);
                rec[6] = (unsigned long long)__double_as_longlong(p.z);
                rec[7] = (unsigned long long)__double_as_longlong(q.x); rec[8] = (unsigned long long)__double_as_longlong(q.y);
                rec[9] = (unsigned long long)__double_as_longlong(q.z); rec[10] = (unsigned long long)__double_as_longlong(q.w);
            } else {
                const int e0 = 6 * (b - mm);                                // clone n - mm = entry block b - mm of the span
                const fixp_rt E0 = fixp_ld(chain, mm - a - 1), E1 = fixp_ld(chain, mm - a);
                m33 Z;
#pragma unroll
                for (int i = 0; i < 9; ++i) Z.m[i] = 0.0;
                wedge_put33(Hs, e0, 0, scl33(-1.0, mul33(mul33(Bkt, skew33(sub3(l, E0.t))), E0.A))); wedge_put33(Hs, e0 + 3, 0, mul33(Bkt, E1.A));
                wedge_put33(Hs, e0, 3, E0.A); wedge_put33(Hs, e0 + 3, 3, Z);
            }
        }
    }
    __syncthreads();

    // ---- 3  T = P_span H^T, Ts[entry * 6 + column]
    for (int e = tid; e < nz; e += LP_WEDGE_T) {
        const double* pc = P + c0 + e;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int c = 0; c < nz; ++c) {
            const double pv = pc[(size_t)(c0 + c) * ld];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[r] = fma(pv, Hs[c * 6 + r], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) Ts[e * 6 + r] = acc[r];
    }
    __syncthreads();

    // ---- 4  C = H T: the shares of the seven groups, then their sum in a fixed order
    if (tid < LP_WEDGE_GROUPS * 36) {
        const int g = tid / 36, ent = tid - 36 * g, i = ent / 6, j = ent - 6 * i;
        double cij = 0.0, cji = 0.0;
        for (int e = g; e < nz; e += LP_WEDGE_GROUPS) {
            cij = fma(Hs[e * 6 + i], Ts[e * 6 + j], cij);
            cji = fma(Hs[e * 6 + j], Ts[e * 6 + i], cji);
        }
        part[2 * tid] = cij; part[2 * tid + 1] = cji;
    }
    __syncthreads();
    if (tid < 36) {
        double cij = part[2 * tid], cji = part[2 * tid + 1];
#pragma unroll
        for (int g = 1; g < LP_WEDGE_GROUPS; ++g) { cij += part[2 * (36 * g + tid)]; cji += part[2 * (36 * g + tid) + 1]; }
        rec[11 + tid] = (unsigned long long)__double_as_longlong(0.5 * (cij + cji));
    }
    __syncthreads();

    // ---- 5  the record
    if (tid < LP_WEDGE_WORDS) out[tid] = rec[tid];
}

// ---- window_joint_kernel.  With J_a window_pose_kernel's Jacobian at age a, the joint covariance of the world poses of the ages 0 .. m - 1 is the
// 6 m x 6 m matrix of the blocks X_ab = J_a P J_b^T, in pose_cov's order and error convention block by block, frames newest first.
//
// Grid (ages, 1, instances), ONE workgroup of LP_WJNT_T = 256 threads per (instance, age).  Workgroup a runs steps 1 - 5 of window_pose_kernel as
// they stand there — the chain, J_a staged, T_a = P_nz J_a^T, the diagonal block (C + C^T) / 2 by the same reduction, the record — so the
// diagonal block and the rvio_window_pose record carry the bits rvio_hip_get_window gives.  Then, for b = 0 .. a - 1 in turn:
//   6  J_b staged from the same chain at the entries of a's compacted set (the columns of J_b that are not zero are a subset of J_a's: the head
//      and the clones n - b .. n - 1, entries 0 .. 5 and 6 + 6 (a - b) .. 6 + 6 a - 1)
//   7  X_ba = J_b T_a: thread (g, entry (i, j)) its share over the f = g, g + 7, ... of J_b's 6 + 6 b entries in rising order; thread entry adds the
//      seven shares in the order 0 .. 6 and stores the sum to block (b, a) at (i, j) AND to block (a, b) at (j, i): every off-diagonal pair is
//      written from one value by one workgroup, so the matrix is symmetric bit for bit
// It reads what window_pose_kernel reads at age a.  An age outside 0 .. n: the pose record of the img_count = -1 form, and 0.0 in the blocks
// (b, a) and (a, b) of every b <= a (an age inside the window never writes a block that touches one outside).
//
// poses: record (z, a) at poses[z * pose_stride + a]; cov: instance z's matrix cov_stride doubles behind instance 0's, row-major, leading
// dimension ldc >= 6 gridDim.x
__global__ __launch_bounds__(LP_WJNT_T) void window_joint_kernel(int n, int ld, const double* __restrict__ x, const double* __restrict__ P, size_t bs,
                                                                 int ref_count, unsigned long long* __restrict__ poses, size_t pose_stride,
                                                                 double* __restrict__ cov, size_t cov_stride, int ldc) {
    static_assert(LP_WJNT_T == 256 && LP_FIXP_NMAX < 64 && LP_WINP_GROUPS * 36 <= LP_WJNT_T && LP_WINP_WORDS <= LP_WJNT_T, "four waves, one lane per clone");
    __shared__ double chain[LP_FIXP_CHAIN];
    __shared__ __align__(16) double Js[LP_WINP_NZ * 6];
    __shared__ __align__(16) double Ts[LP_WINP_NZ * 6];
    __shared__ __align__(16) double Jb[LP_WINP_NZ * 6];
    __shared__ double part[LP_WINP_GROUPS * 36 * 2];
    __shared__ double partb[LP_WINP_GROUPS * 36];
    __shared__ unsigned long long rec[LP_WINP_WORDS];
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int a = (int)blockIdx.x;
    unsigned long long* out = poses + (size_t)z * pose_stride * LP_WINP_WORDS + (size_t)a * LP_WINP_WORDS;
    cov += (size_t)z * cov_stride;
    if (!(n >= 0 && n <= LP_FIXP_NMAX && a <= n)) {
        if (tid < LP_WINP_WORDS) {
            unsigned long long w = 0ull;
            if (tid == 1) w = 0xffffffffull;                              // img_count = -1, age = 0
            if (tid == 2) w = (unsigned long long)(unsigned)n;            // n_clones, reserved = 0
            out[tid] = w;
        }
        for (int e = tid; e < 36 * (a + 1); e += LP_WJNT_T) {             // the blocks (b, a) and (a, b), b = 0 .. a
            const int bb = e / 36, ent = e - 36 * bb, i = ent / 6, j = ent - 6 * i;
            cov[(size_t)(6 * bb + i) * ldc + 6 * a + j] = 0.0;
            cov[(size_t)(6 * a + j) * ldc + 6 * bb + i] = 0.0;
        }
        return;
    }
    x = zoffi(x, bs, z);
    P = zoffi(P, bs, z);

    // ---- 1  the chain (window_pose_kernel's step 1)
    {
        const int mm = lane + 1;
        fixp_rt e;
        e.A = eye33(); e.t = mk3(0.0, 0.0, 0.0);
        if (mm <= a) {
            const double* c = x + 26 + 7 * (n - mm);
            e.A = q2r(ldq(c));
            e.t = scl3(-1.0, mv33(e.A, ld3(c + 4)));
        }
        for (int off = 1; off < a; off <<= 1) {          // (uniform: a is the workgroup's)
            fixp_rt o;
#pragma unroll
            for (int k = 0; k < 9; ++k) o.A.m[k] = __shfl_up(e.A.m[k], off, 64);
            o.t.x = __shfl_up(e.t.x, off, 64); o.t.y = __shfl_up(e.t.y, off, 64); o.t.z = __shfl_up(e.t.z, off, 64);
            if (lane >= off) { e.t = add3(o.t, mv33(o.A, e.t)); e.A = mul33(o.A, e.A); }
        }
        if (wv == 0 && mm <= a) {
            double* c = chain + 12 * mm;
#pragma unroll
            for (int k = 0; k < 9; ++k) c[k] = e.A.m[k];
            c[9] = e.t.x; c[10] = e.t.y; c[11] = e.t.z;
        }
        if (tid == 63) {
#pragma unroll
            for (int k = 0; k < 12; ++k) chain[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        }
    }
    __syncthreads();

    // ---- 2  J_a (window_pose_kernel's step 2)
    const int nz = 6 + 6 * a, c0 = 24 + 6 * (n - a);
    if (tid < a || tid == 64) {
        const m33 RG = q2r(ldq(x));
        const m33 RGt = tr33(RG);
        const fixp_rt Ea = fixp_ld(chain, a);
        m33 Z;
#pragma unroll
        for (int k = 0; k < 9; ++k) Z.m[k] = 0.0;
        if (tid == 64) {
            const d3 sa = sub3(Ea.t, ld3(x + 4));
            winp_put33(Js, 0, 0, scl33(-1.0, mul33(RGt, skew33(sa)))); winp_put33(Js, 3, 0, scl33(-1.0, RGt));
            winp_put33(Js, 0, 3, RGt); winp_put33(Js, 3, 3, Z);
            const d3 p = mv33(RGt, sa);
            const q4 q = a == 0 ? ldq(x) : r2q(mul33(tr33(Ea.A), RG));
            rec[0] = 0ull;
            rec[1] = (unsigned long long)(unsigned)(ref_count - a) | ((unsigned long long)(unsigned)a << 32);
            rec[2] = (unsigned long long)(unsigned)n;
            rec[3] = (unsigned long long)__double_as_longlong(p.x); rec[4] = (unsigned long long)__double_as_longlong(p.y);
            rec[5] = (unsigned long long)__double_as_longlong(p.z);
            rec[6] = (unsigned long long)__double_as_longlong(q.x); rec[7] = (unsigned long long)__double_as_longlong(q.y);
            rec[8] = (unsigned long long)__double_as_longlong(q.z); rec[9] = (unsigned long long)__double_as_longlong(q.w);
        } else {
            const int mm = tid + 1, e0 = 6 + 6 * (a - mm);              // clone n - mm = entry block a - mm of the compacted set
            const fixp_rt E0 = fixp_ld(chain, mm - 1), E1 = fixp_ld(chain, mm);
            winp_put33(Js, e0, 0, mul33(mul33(RGt, skew33(sub3(Ea.t, E0.t))), E0.A)); winp_put33(Js, e0 + 3, 0, scl33(-1.0, mul33(RGt, E1.A)));
            winp_put33(Js, e0, 3, scl33(-1.0, mul33(RGt, E0.A))); winp_put33(Js, e0 + 3, 3, Z);
        }
    }
    __syncthreads();

    // ---- 3  T_a = P_nz J_a^T (window_pose_kernel's step 3)
    for (int e = tid; e < nz; e += LP_WJNT_T) {
        const double* pc = P + winp_col(e, c0);
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k = 0; k < nz; ++k) {
            const double pv = pc[(size_t)winp_col(k, c0) * ld];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[r] = fma(pv, Js[k * 6 + r], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) Ts[e * 6 + r] = acc[r];
    }
    __syncthreads();

    // ---- 4  the diagonal block (window_pose_kernel's step 4)
    if (tid < LP_WINP_GROUPS * 36) {
        const int g = tid / 36, ent = tid - 36 * g, i = ent / 6, j = ent - 6 * i;
        double cij = 0.0, cji = 0.0;
        for (int e = g; e < nz; e += LP_WINP_GROUPS) {
            cij = fma(Js[e * 6 + i], Ts[e * 6 + j], cij);
            cji = fma(Js[e * 6 + j], Ts[e * 6 + i], cji);
        }
        part[2 * tid] = cij; part[2 * tid + 1] = cji;
    }
    __syncthreads();
    if (tid < 36) {
        double cij = part[2 * tid], cji = part[2 * tid + 1];
#pragma unroll
        for (int g = 1; g < LP_WINP_GROUPS; ++g) { cij += part[2 * (36 * g + tid)]; cji += part[2 * (36 * g + tid) + 1]; }
        const double c = 0.5 * (cij + cji);
        rec[10 + tid] = (unsigned long long)__double_as_longlong(c);
        const int i = tid / 6, j = tid - 6 * i;
        cov[(size_t)(6 * a + i) * ldc + 6 * a + j] = c;
    }
    __syncthreads();

    // ---- 5  the record
    if (tid < LP_WINP_WORDS) out[tid] = rec[tid];

    // ---- 6, 7  the blocks (b, a) and (a, b) of the newer frames b < a
    for (int b = 0; b < a; ++b) {
        const int nzb = 6 + 6 * b, eb = 6 + 6 * (a - b);                  // J_b's clone entries start at eb of a's set
        if (tid < b || tid == 64) {
            const m33 RGt = tr33(q2r(ldq(x)));
            const fixp_rt Eb = fixp_ld(chain, b);
            m33 Z;
#pragma unroll
            for (int k = 0; k < 9; ++k) Z.m[k] = 0.0;
            if (tid == 64) {
                const d3 sb = sub3(Eb.t, ld3(x + 4));
                winp_put33(Jb, 0, 0, scl33(-1.0, mul33(RGt, skew33(sb)))); winp_put33(Jb, 3, 0, scl33(-1.0, RGt));
                winp_put33(Jb, 0, 3, RGt); winp_put33(Jb, 3, 3, Z);
            } else {
                const int mm = tid + 1, e0 = 6 + 6 * (a - mm);
                const fixp_rt E0 = fixp_ld(chain, mm - 1), E1 = fixp_ld(chain, mm);
                winp_put33(Jb, e0, 0, mul33(mul33(RGt, skew33(sub3(Eb.t, E0.t))), E0.A)); winp_put33(Jb, e0 + 3, 0, scl33(-1.0, mul33(RGt, E1.A)));
                winp_put33(Jb, e0, 3, scl33(-1.0, mul33(RGt, E0.A))); winp_put33(Jb, e0 + 3, 3, Z);
            }
        }
        __syncthreads();
        if (tid < LP_WINP_GROUPS * 36) {
            const int g = tid / 36, ent = tid - 36 * g, i = ent / 6, j = ent - 6 * i;
            double s = 0.0;
            for (int f = g; f < nzb; f += LP_WINP_GROUPS) {
                const int e = f < 6 ? f : eb + f - 6;
                s = fma(Jb[e * 6 + i], Ts[e * 6 + j], s);
            }
            partb[tid] = s;
        }
        __syncthreads();
        if (tid < 36) {
            double s = partb[tid];
#pragma unroll
            for (int g = 1; g < LP_WINP_GROUPS; ++g) s += partb[36 * g + tid];
            const int i = tid / 6, j = tid - 6 * i;
            cov[(size_t)(6 * b + i) * ldc + 6 * a + j] = s;
            cov[(size_t)(6 * a + j) * ldc + 6 * b + i] = s;
        }
        // (the next b's stage writes Jb and partb: behind the reads above only after a barrier)
        __syncthreads();
    }
}
