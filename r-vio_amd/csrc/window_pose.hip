// window_pose.hip — the fixed-lag smoothed trajectory (rvio_window_pose of include/rvio_hip.h): the world pose of the IMU at the image `age` frames
// back from the state's reference frame {R}, composed from (qG, pG) and the newest `age` clones AS THEY ARE NOW — every camera update, delayed
// fix, relative-pose measurement and map observation since has corrected them — and its 6 x 6 covariance, which follows from P.
//
// Frames and chain are those of fix_past.hip: clone i holds (q_i, p_i), C_i = R(q_i), the age a = 0 .. n counts images back from {R},
//   A_0 = I, t_0 = 0;   A_m = A_{m-1} C_{n-m},   t_m = t_{m-1} - A_m p_{n-m}      (m = 1 .. a)
// With R_G = R(qG) and lever 0:
//   p    = R_G^T (t_a - pG)                        the world position of the IMU at that image
//   R(q) = A_a^T R_G                               world -> IMU at that image
//   J    = the three POSITION rows (lever 0, frac 0) over the three ATTITUDE rows of the past-fix table at age a (6 x d):
//     cols 0-2: -R_G^T [(t_a - pG) x] | R_G^T     3-5: -R_G^T | 0
//     clone n - m (m = 1 .. a):   rotation  R_G^T [(t_a - t_{m-1}) x] A_{m-1} | -R_G^T A_{m-1}     position  -R_G^T A_m | 0
//   pose_cov = (C + C^T) / 2,  C = J P J^T         order and error convention of rvio_odom.pose_cov; at a = 0 J is odom.hip's map
// The sign of q: at a = 0 the bits of x[0..3] (what the pose line and rvio_odom.q carry); at a > 0 RotToQuat's, normalised with q[3] >= 0.
//
// Grid (ages, 1, instances), ONE workgroup of LP_WINP_T = 256 threads per (instance, age), FP64, plain C++, static LDS only, no atomics.
//   1  every wave forms the chain by the in-wave scan of fix_past_kernel (lane m - 1 <-> clone n - m); wave 0 drops it into LDS
//   2  the columns of J that are not zero — 0 .. 5 and 24 + 6 (n - a) .. 24 + 6 n - 1, k = 6 + 6 a <= LP_WINP_NZ of them — staged in LDS as
//      Js[entry][row]: thread m - 1 the six columns of clone n - m, thread 64 the head
//   3  T = P_nz J^T: thread <-> entry e of the compacted set (a loop: k exceeds one wave), six accumulators, a loop over the other index.  P is
//      symmetric and column-major, so consecutive threads read consecutive doubles of one column of P per load; the row of J is a broadcast
//   4  C = J T: thread (g, entry) with entry = (i, j) of the 36 and g one of LP_WINP_GROUPS = 7 groups that take the e = g, g + 7, ... in rising
//      order; it forms its share of C_ij AND of C_ji.  Thread entry then adds the seven shares in the order 0 .. 6 and halves the sum of the two:
//      entry (i, j) and its mirror (j, i) add the same two numbers in either order, hence the same bits; the same bits every run
//   5  the 46 words of the record from LDS: one coalesced store
// It reads x[0..6], the newest a clones and the rows / columns of P named in 2; it writes its record, nothing else.
// An age outside 0 .. n: img_count = -1, n_clones set, every other word 0.
__device__ __forceinline__ int winp_col(int e, int c0) { return e < 6 ? e : c0 + e - 6; }   // column of entry e of the compacted non-zero set
__device__ __forceinline__ void winp_put33(double* Js, int e0, int row0, const m33& X) {   // block X at entries e0 .. e0 + 2, rows row0 .. row0 + 2
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Js[(e0 + j) * 6 + row0 + i] = X.m[3 * i + j];
}

// x / P: instance 0's, instance z lies bs bytes behind; ld: leading dimension of P; n: clones now; the workgroup (b, 0, z) forms the record of age
// age_first + b of instance z into out[z * out_stride + b]; ref_count: the frame count of {R}
__global__ __launch_bounds__(LP_WINP_T) void window_pose_kernel(int n, int ld, const double* __restrict__ x, const double* __restrict__ P, size_t bs,
                                                                int age_first, int ref_count, long long seq, unsigned long long* __restrict__ out,
                                                                size_t out_stride) {
    static_assert(LP_WINP_T == 256 && LP_FIXP_NMAX < 64 && LP_WINP_GROUPS * 36 <= LP_WINP_T && LP_WINP_WORDS <= LP_WINP_T, "four waves, one lane per clone");
    __shared__ double chain[LP_FIXP_CHAIN];
    __shared__ __align__(16) double Js[LP_WINP_NZ * 6];
    __shared__ __align__(16) double Ts[LP_WINP_NZ * 6];
    __shared__ double part[LP_WINP_GROUPS * 36 * 2];
    __shared__ unsigned long long rec[LP_WINP_WORDS];
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int a = age_first + (int)blockIdx.x;
    out += (size_t)z * out_stride * LP_WINP_WORDS + (size_t)blockIdx.x * LP_WINP_WORDS;
    if (!(n >= 0 && n <= LP_FIXP_NMAX && a >= 0 && a <= n)) {
        if (tid < LP_WINP_WORDS) {
            unsigned long long w = 0ull;
            if (tid == 1) w = 0xffffffffull;                              // img_count = -1, age = 0
            if (tid == 2) w = (unsigned long long)(unsigned)n;            // n_clones, reserved = 0
            out[tid] = w;
        }
        return;
    }
    x = zoffi(x, bs, z);
    P = zoffi(P, bs, z);

    // ---- 1  the chain: lane m - 1 holds the element of clone n - m, the identity where the chain does not reach
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

    // ---- 2  the columns of J that are not zero, Js[entry * 6 + row]; thread 64 also forms p, q and the counts
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
            rec[0] = (unsigned long long)seq;
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

    // ---- 3  T = P_nz J^T, Ts[entry * 6 + column]
    for (int e = tid; e < nz; e += LP_WINP_T) {
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

    // ---- 4  C = J T: the shares of the seven groups, then their sum in a fixed order
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
        rec[10 + tid] = (unsigned long long)__double_as_longlong(0.5 * (cij + cji));
    }
    __syncthreads();

    // ---- 5  the record
    if (tid < LP_WINP_WORDS) out[tid] = rec[tid];
}
