// imu_pose.hip — IMU-rate odometry (rvio_imu_pose of include/rvio_hip.h): the pose line System::MonoVIO would write if an image arrived right
// behind IMU sample j and that frame ran no update, for EVERY sample of a batch.  PreIntegrator::propagate has (Rk, pk, vk) complete at the
// bottom of every iteration of its sample loop (PreIntegrator.cc:168-176) and keeps the last; this kernel keeps them all.  States only: no
// Phi, no Q, no P.
//
// Launched by rvio_hip_predict[_dev] (records of a batch from the handle's current state, no side effect) and, when the IMU-rate ring is
// enabled (rvio_hip_set_imu_odometry), directly in front of whatever propagates in place.  It reads x[0..25] and the IMU batch, writes records.
//
// Geometry (launch_plan.h LP_IMUP_*): one wave per instance, four instances per 256-thread workgroup, no block-wide barrier — odom_kernel's.
// Per chunk of up to 64 samples a wave runs
//   A  lane s <-> sample s: trig, dR, f1..f4 and the two a-dependent vectors — the expressions of propagate_body's phase A, term for term
//   B  the serial chain over the chunk in the reference's order, every lane redundantly (uniform operands, no divergence): Rk <- dR Rk, dp, dv, Dt.
//      Its state carries across chunks in registers.  pk and vk are functions of (Rk, dp, dv, Dt) and of the start state only — nothing of
//      the chain depends on them —, so they are formed in phase C, in parallel, by the expressions propagate_body has in its chain
//   C  lane s <-> record s: pk, vk, RotToQuat(Rk), QuatMul with qG, R(qG)^T (pk - pG) with the device functions augcomp_kernel2 uses
// Sample s's (dR, up, uv, dt) reach the chain through LDS: 16 doubles per sample, word-major (word k of sample s at [k][s]) = 8 KB per wave.
// Lane-indexed accesses (phases A, C) are then consecutive 8-byte words — conflict-free —, the chain's reads have a wave-uniform address —
// one broadcast each, issued ahead of the dependent arithmetic of the step.  Step s overwrites ITS sample's 16 words with (Rk, dp, dv, Dt)
// behind that step (one lane stores): LDS operations of one wave complete in order, so no barrier.  Cross-lane reads (v_readlane) instead
// would be 32 scalar-indexed reads per step on the chain's own issue port plus 32 selects per step to leave "lane s keeps step s" behind —
// more instructions on the one wave's serial path than 16 broadcast loads and 16 stores that the LDS pipeline takes off it.
// Register arrays are indexed by compile-time constants only (the rule at the head of filter_kernels2.hip).
#define IMUP_WORDS 13   // sizeof(rvio_imu_pose) / 8
#define IMUP_SLOT(W, k, s) (W)[(k) * 64 + (s)]

// out: predict (cap == 0): record j of instance z at out[z * out_stride + j], seq 0; ring (cap > 0): record j has seq = seq0 + j and goes to
// slot (seq - 1) % cap of ring[cap][batch] — of a batch longer than the ring only the last cap records are stored (two records of one launch
// never share a slot).  x / imu: instance 0's; instance z lies z * bs / z * imu_bs bytes behind (imu_bs = 0: one shared batch).
__global__ __launch_bounds__(LP_IMUP_T) void imu_pose_kernel(double small_angle, double nG, int batch, const double* __restrict__ x, size_t bs,
                                                             const rvio_imu* __restrict__ imu, size_t imu_bs, int m,
                                                             unsigned long long* __restrict__ out, long long out_stride, long long seq0, int cap,
                                                             int img_count) {
    extern __shared__ __align__(16) double imup_dyn[];
    const int wv = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z = (int)blockIdx.x * LP_IMUP_WAVES + wv;
    if (z >= batch) return;
    double* W = imup_dyn + wv * (LP_IMUP_WAVE_BYTES / 8);
    x = zoffi(x, bs, z); imu = zoffi(imu, imu_bs, z);
    const q4 qG = ldq(x);
    const d3 pG = ld3(x + 4);
    const d3 bg = ld3(x + 20), ba = ld3(x + 23);
    const d3 gR = ld3(x + 7), vR = ld3(x + 17);
    const m33 I = eye33();
    // the chain's state
    m33 Rk = q2r(ldq(x + 10)), RkT = tr33(Rk);
    d3 dp = mk3(0, 0, 0), dv = mk3(0, 0, 0);
    double Dt = 0.0;
    for (int s0 = 0; s0 < m; s0 += 64) {
        const int mc = (m - s0 < 64) ? (m - s0) : 64;
        // ---- A
        double t_s = 0.0;
        if (lane < mc) {
            const rvio_imu u = imu[s0 + lane];
            const d3 w = sub3(mk3(u.w[0], u.w[1], u.w[2]), bg), a = sub3(mk3(u.a[0], u.a[1], u.a[2]), ba);
            const double dt = u.dt, w1 = nrm3(w);
            const bool small = w1 < small_angle;
            const double wdt = w1 * dt, wdt2 = wdt * wdt;
            double sw, cw;
            sincos(wdt, &sw, &cw);
            const m33 wx = skew33(w), wx2 = mul33(wx, wx);
            m33 dR; double f1, f2, f3, f4;
            if (small) {
                dR = add33(sub33(I, scl33(dt, wx)), scl33(dt * dt / 2, wx2));
                f1 = -(dt * dt * dt) / 3; f2 = (dt * dt * dt * dt) / 8; f3 = -(dt * dt) / 2; f4 = (dt * dt * dt) / 6;
            } else {
                const double w2 = w1 * w1, w3 = w2 * w1, w4 = w2 * w2;
                dR = add33(sub33(I, scl33(sw / w1, wx)), scl33((1 - cw) / w2, wx2));
                f1 = (wdt * cw - sw) / w3;
                f2 = .5 * (wdt2 - 2 * cw - 2 * wdt * sw + 2) / w4;
                f3 = (cw - 1) / w2;
                f4 = (wdt - sw) / w3;
            }
            const d3 up = mv33(add33(add33(scl33(.5 * dt * dt, I), scl33(f1, wx)), scl33(f2, wx2)), a);
            const d3 uv = mv33(add33(add33(scl33(dt, I), scl33(f3, wx)), scl33(f4, wx2)), a);
#pragma unroll
            for (int k = 0; k < 9; ++k) IMUP_SLOT(W, k, lane) = dR.m[k];
            IMUP_SLOT(W, 9, lane) = up.x; IMUP_SLOT(W, 10, lane) = up.y; IMUP_SLOT(W, 11, lane) = up.z;
            IMUP_SLOT(W, 12, lane) = uv.x; IMUP_SLOT(W, 13, lane) = uv.y; IMUP_SLOT(W, 14, lane) = uv.z;
            IMUP_SLOT(W, 15, lane) = dt;
            t_s = u.t;
        }
        // (one wave: its LDS operations complete in program order; the fence keeps the compiler from moving them across the phase boundary)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- B
        for (int s = 0; s < mc; ++s) {
            m33 dR;
#pragma unroll
            for (int k = 0; k < 9; ++k) dR.m[k] = IMUP_SLOT(W, k, s);
            const d3 up = mk3(IMUP_SLOT(W, 9, s), IMUP_SLOT(W, 10, s), IMUP_SLOT(W, 11, s));
            const d3 uv = mk3(IMUP_SLOT(W, 12, s), IMUP_SLOT(W, 13, s), IMUP_SLOT(W, 14, s));
            const double dt = IMUP_SLOT(W, 15, s);
            Dt += dt;
            Rk = mul33(dR, Rk); RkT = tr33(Rk);
            dp = add3(dp, scl3(dt, dv));
            dp = add3(dp, mv33(RkT, up));
            dv = add3(dv, mv33(RkT, uv));
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) IMUP_SLOT(W, k, s) = Rk.m[k];
                IMUP_SLOT(W, 9, s) = dp.x; IMUP_SLOT(W, 10, s) = dp.y; IMUP_SLOT(W, 11, s) = dp.z;
                IMUP_SLOT(W, 12, s) = dv.x; IMUP_SLOT(W, 13, s) = dv.y; IMUP_SLOT(W, 14, s) = dv.z;
                IMUP_SLOT(W, 15, s) = Dt;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- C
        const int j = s0 + lane;
        if (lane < mc && (cap == 0 || j >= m - cap)) {
            m33 Rs;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rs.m[k] = IMUP_SLOT(W, k, lane);
            const d3 dps = mk3(IMUP_SLOT(W, 9, lane), IMUP_SLOT(W, 10, lane), IMUP_SLOT(W, 11, lane));
            const d3 dvs = mk3(IMUP_SLOT(W, 12, lane), IMUP_SLOT(W, 13, lane), IMUP_SLOT(W, 14, lane));
            const double Dts = IMUP_SLOT(W, 15, lane);
            // (pk, vk: the expressions of propagate_body's chain, formed here.  That the compiler contracts them as it does there is what
            // tests/test_gpu_imu_odometry.py test_last_record_has_the_bits_of_propagate guards: change neither side without it)
            const d3 pk = add3(sub3(scl3(Dts, vR), scl3(.5 * nG * Dts * Dts, gR)), dps);
            const d3 vk = mv33(Rs, add3(sub3(vR, scl3(nG * Dts, gR)), dvs));
            const q4 qk = r2q(Rs);
            const q4 qkG = qmul(qk, qG);
            const d3 pGk = mv33(tr33(q2r(qG)), sub3(pk, pG));   // pose line (System.cc:371-374)
            const long long seq = cap ? seq0 + j : 0;
            const size_t rec = cap ? (size_t)((seq - 1) % cap) * (size_t)batch + (size_t)z : (size_t)z * (size_t)out_stride + (size_t)j;
            unsigned long long* o = out + rec * IMUP_WORDS;
            o[0] = (unsigned long long)seq;
            o[1] = (unsigned long long)(unsigned)img_count | ((unsigned long long)(unsigned)j << 32);
            o[2] = (unsigned long long)__double_as_longlong(t_s);
            o[3] = (unsigned long long)__double_as_longlong(pGk.x); o[4] = (unsigned long long)__double_as_longlong(pGk.y); o[5] = (unsigned long long)__double_as_longlong(pGk.z);
            o[6] = (unsigned long long)__double_as_longlong(qkG.x); o[7] = (unsigned long long)__double_as_longlong(qkG.y);
            o[8] = (unsigned long long)__double_as_longlong(qkG.z); o[9] = (unsigned long long)__double_as_longlong(qkG.w);
            o[10] = (unsigned long long)__double_as_longlong(vk.x); o[11] = (unsigned long long)__double_as_longlong(vk.y); o[12] = (unsigned long long)__double_as_longlong(vk.z);
        }
        // (the next chunk's phase A rewrites the slots phase C has read: same wave, program order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
