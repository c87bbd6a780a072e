// standstill.hip — standstill detection (rvio_hip_standstill[_dev] of include/rvio_hip.h): per instance, from the IMU batch of the frame, the
// biases in x and the last two observations of every live track, the decision "the platform does not move", made where that data lies and
// handed to aux_update_kernel as its per-instance `active` flag together with the measurement of the zero-velocity (+ gyro-bias) update.
//
// One launch, gridDim.z = instances, ONE workgroup of LP_SS_T threads (four waves) per instance.
//   IMU statistic (SHOE / GLRT, Skog et al. 2010 — no attitude in it, hence no sign convention):
//     a^_j = a_j - ba,  w^_j = w_j - bg,  a_ = (1/m) sum a^_j,  u = a_ / |a_|
//     T = (1/m) sum_j ( |a^_j - G u|^2 / sigma_a^2 + |w^_j|^2 / sigma_w^2 )
//   in TWO passes over the samples (the one-pass form sum |a^|^2 - 2 G m |a_| + m G^2 cancels ~ G^2 / sigma^2 against itself).
//   Image statistic (handles with a front end): over the live points i < *n_pts with hist_len[slot[i]] >= 2 the mean of
//     sqrt((fx dx)^2 + (fy dy)^2),  (dx, dy) = hist[s][hl - 1] - hist[s][hl - 2]  (float32 normalised coordinates, widened to double)
//   with the INSTANCE's calibration (cam_of).  It can only veto: too few pairs = no opinion.
// Reductions: strided per-thread partial sums, wave_sum (DPP, fixed order), then the four waves' sums through static LDS, added in the order
// (w0 + w1) + (w2 + w3) by every thread: no floating-point atomics, nothing that depends on timing — two runs of the same inputs give the same
// bits.  All arithmetic is FP64.
// One thread stores the record, the flag active[z] = is_static && apply, v[z] = (0, 0, 0, mean raw gyro) and clears the instance's (gamma,
// applied) pair, which aux_update_kernel rewrites when it runs; the workgroup of instance 0 also writes the shared H (rows x d, row-major,
// ones at (r, 15 + r): velocity columns 15..17, gyro-bias columns 18..20) and sigma.
// Every index read from the tracker's tables is clamped to the table it addresses: a poisoned table gives a wrong statistic, never a stray load.

// the sums of the four waves, combined in a fixed order; every thread returns the same bits.  (red: LP_SS_RED x LP_SS_WAVES doubles)
template <int K>
__device__ __forceinline__ void ss_block_sum(double (&v)[K], double* red) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    __syncthreads();   // (the previous round's reads of `red` are done)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[k * LP_SS_WAVES + wv] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k * LP_SS_WAVES] + red[k * LP_SS_WAVES + 1]) + (red[k * LP_SS_WAVES + 2] + red[k * LP_SS_WAVES + 3]);
}

// x: instance 0's state, instance z lies bs bytes behind (as the tracker's tables); imu: instance 0's samples, imu_bs BYTES between instances
// (0: shared); front: the handle has a front end (t is valid); n: clones in the window now; rows: 3 | 6
__global__ __launch_bounds__(LP_SS_T) void standstill_kernel(DevCfg cfg, const CamCal* __restrict__ cal, TrackerDev t, int front, const double* x, size_t bs,
                                                             const rvio_imu* imu, size_t imu_bs, int m, rvio_standstill_config c, int n, int rows, int apply,
                                                             int img_count, rvio_standstill* rec, int* active, double* v, double* H, double* sigma,
                                                             double* diag) {
    static_assert(LP_SS_WAVES == 4, "ss_block_sum adds four waves");
    __shared__ double red[LP_SS_RED * LP_SS_WAVES];
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x;
    x = zoffi(x, bs, z);
    imu = zoffi(imu, imu_bs, z);
    const double bgx = x[20], bgy = x[21], bgz = x[22], bax = x[23], bay = x[24], baz = x[25];
    // ---- pass 1: the mean specific force and the mean rate
    double s1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < m; j += LP_SS_T) {
        const rvio_imu s = imu[j];
        s1[0] += s.a[0] - bax; s1[1] += s.a[1] - bay; s1[2] += s.a[2] - baz;
        s1[3] += s.w[0] - bgx; s1[4] += s.w[1] - bgy; s1[5] += s.w[2] - bgz;
    }
    ss_block_sum<6>(s1, red);
    const double rm = 1.0 / (double)m;
    const double ax = s1[0] * rm, ay = s1[1] * rm, az = s1[2] * rm;
    const double an = sqrt(ax * ax + ay * ay + az * az);
    const double gx = cfg.gravity * (ax / an), gy = cfg.gravity * (ay / an), gz = cfg.gravity * (az / an);
    // ---- pass 2: the statistic
    const double isa = 1.0 / (c.sigma_a * c.sigma_a), isw = 1.0 / (c.sigma_w * c.sigma_w);
    double s2[1] = {0.0};
    for (int j = tid; j < m; j += LP_SS_T) {
        const rvio_imu s = imu[j];
        const double ex = (s.a[0] - bax) - gx, ey = (s.a[1] - bay) - gy, ez = (s.a[2] - baz) - gz;
        const double wx = s.w[0] - bgx, wy = s.w[1] - bgy, wz = s.w[2] - bgz;
        s2[0] += (ex * ex + ey * ey + ez * ez) * isa + (wx * wx + wy * wy + wz * wz) * isw;
    }
    ss_block_sum<1>(s2, red);
    const double T = s2[0] * rm;
    const bool imu_static = an > 0.0 && T < c.imu_thr;   // (a NaN compares false)
    // ---- the image statistic
    double s3[2] = {0.0, 0.0};   // sum of the steps (px), their count (exact in a double: <= F)
    if (front) {
        tracker_shift(t, (size_t)z * bs);
        const CamCal cam = cam_of(cfg, cal, z);
        const double fx = (double)cam.fx, fy = (double)cam.fy;
        const int F = cfg.F, ML = cfg.max_len;
        const int N = min(max(*t.n_pts, 0), F);
        const float2* hist = (const float2*)t.hist;
        for (int i = tid; i < N; i += LP_SS_T) {
            const int s = min(max(t.slot[i], 0), F - 1);
            const int hl = min(t.hist_len[s], ML);
            if (hl >= 2) {
                const float2 p1 = hist[(size_t)s * ML + hl - 1], p0 = hist[(size_t)s * ML + hl - 2];
                const double dx = fx * ((double)p1.x - (double)p0.x), dy = fy * ((double)p1.y - (double)p0.y);
                s3[0] += sqrt(dx * dx + dy * dy);
                s3[1] += 1.0;
            }
        }
        ss_block_sum<2>(s3, red);
    }
    const int n_pairs = (int)s3[1];
    const double disparity = n_pairs > 0 ? s3[0] / s3[1] : 0.0;
    const bool img_static = !(c.disp_thr_px > 0.0) || n_pairs < c.min_pairs || disparity < c.disp_thr_px;
    const bool is_static = imu_static && img_static;
    if (tid == 0) {
        rvio_standstill r;
        r.T = T; r.disparity = disparity; r.gamma = 0.0;
        r.n_pairs = n_pairs; r.flags = (imu_static ? 1 : 0) | (img_static ? 2 : 0) | (is_static ? 4 : 0);
        r.m = m; r.img_count = img_count;
        rec[z] = r;
        active[z] = (is_static && apply) ? 1 : 0;
        double* vz = v + 6 * (size_t)z;
        vz[0] = 0.0; vz[1] = 0.0; vz[2] = 0.0;
        vz[3] = s1[3] * rm + bgx; vz[4] = s1[4] * rm + bgy; vz[5] = s1[5] * rm + bgz;   // the mean RAW gyro reading: at rest w_m = bg + noise
        diag[2 * (size_t)z] = 0.0; ((long long*)diag)[2 * (size_t)z + 1] = 0;
    }
    if (z == 0) {
        const int d = 24 + 6 * n;
        for (int e = tid; e < rows * d; e += LP_SS_T) { const int r = e / d, col = e - r * d; H[e] = (col == 15 + r) ? 1.0 : 0.0; }
        if (tid < 6) sigma[tid] = tid < 3 ? c.sigma_v : c.sigma_bg;
    }
}
