// odom.hip — the per-frame odometry record (rvio_odom of include/rvio_hip.h): what System::MonoVIO publishes every frame as nav_msgs::Odometry
// (System.cc:402-418: the pose and twist.linear = vk) and appends to its nav_msgs::Path (System.cc:420-434), plus the pose covariance the
// reference leaves at zero.
//
// Launched behind augcomp_kernel2 (augment_compose_dev) when the ring is enabled (rvio_hip_set_odometry).  It reads only what that kernel
// wrote — x_out, P_out and the pose line, all in HBM — and writes one 464-byte record into the handle's ring.  One wave per instance, four
// instances per 256-thread workgroup; no LDS, no barrier.  Lane l < 58 owns the l-th 8-byte word of the record, so a record leaves the wave
// as one coalesced vector store.
//
// pose_cov: the composed state's (qkG, pkG) carries the error (dth, dp) of the reference's injection q <- dq (x) q, dq ~ [dth / 2; 1], p <- p + dp
// (Updater.cc:549-566), i.e. R_true ~ (I - [dth x]) R with R = R(qkG).  The published position is pGk = -R^T pkG and the published attitude
// R_wb = R^T; with the world-frame rotation error phi defined by R_wb,true ~ (I + [phi x]) R_wb
//   [dpGk]   [ R^T [p x]   -R^T ] [dth]
//   [ phi ] = [ R^T          0   ] [dp ]          pose_cov = (C + C^T) / 2,   C = J P6 J^T,   P6 = P_out[0..5][0..5]
// (r-vio_amd/abi.py odom_pose_cov is the NumPy mirror; tests/test_odometry_abi.py checks J against central differences of the injection).
// Every lane keeps R, R^T [p x] and P6 in registers under compile-time indices and picks ITS two rows of J with selects: nothing is indexed
// by the lane number, so nothing spills.  Lane 13 + 6 i + j forms C_ij and C_ji from the same products, in the two orders: the symmetrised
// entry (i, j) and its mirror (j, i) are the same two numbers added in either order, hence the same bits.
#define ODOM_WORDS 58   // sizeof(rvio_odom) / 8

__device__ __forceinline__ double odom_sel3(double a, double b, double c, int i) { return i == 0 ? a : (i == 1 ? b : c); }
// row r of J as six registers
__device__ __forceinline__ void odom_jrow(const m33& R, const m33& M, int r, double row[6]) {
    const bool top = r < 3;
    const int c = top ? r : r - 3;
    // top: [M[c][0..2] | -R^T[c][0..2] = -R[0..2][c]],  bottom: [R^T[c][0..2] = R[0..2][c] | 0]
    const double rc0 = odom_sel3(R.m[0], R.m[1], R.m[2], c), rc1 = odom_sel3(R.m[3], R.m[4], R.m[5], c), rc2 = odom_sel3(R.m[6], R.m[7], R.m[8], c);
    row[0] = top ? odom_sel3(M.m[0], M.m[3], M.m[6], c) : rc0;
    row[1] = top ? odom_sel3(M.m[1], M.m[4], M.m[7], c) : rc1;
    row[2] = top ? odom_sel3(M.m[2], M.m[5], M.m[8], c) : rc2;
    row[3] = top ? -rc0 : 0.0;
    row[4] = top ? -rc1 : 0.0;
    row[5] = top ? -rc2 : 0.0;
}

// ring: slot (seq - 1) % capacity of the handle's ring, `batch` records; x_out / P_out / pose_out: instance 0's, instance z lies z * bs bytes behind
__global__ __launch_bounds__(256) void odom_kernel(int batch, int ld, const double* __restrict__ x_out, const double* __restrict__ P_out,
                                                   const double* __restrict__ pose_out, size_t bs, long long seq, int img_count, int n_clones,
                                                   unsigned long long* __restrict__ ring) {
    const int z = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (z >= batch) return;
    x_out = zoffi(x_out, bs, z); P_out = zoffi(P_out, bs, z); pose_out = zoffi(pose_out, bs, z);
    // the covariance entry of this lane (the lanes outside 13..48 compute entry 0 or 35 along and drop it: no divergence in front of the loads)
    const int e = min(max(lane - 13, 0), 35), i = e / 6, j = e % 6;
    double P6[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) P6[r][c] = P_out[(size_t)r + (size_t)c * ld];
    const m33 R = q2r(ldq(pose_out + 3));                    // qkG: the bits of x_out[0..3]
    const m33 M = mul33(tr33(R), skew33(ld3(x_out + 4)));    // R^T [pkG x]
    double ri[6], rj[6];
    odom_jrow(R, M, i, ri);
    odom_jrow(R, M, j, rj);
    double cij = 0.0, cji = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double tj = 0.0, ti = 0.0;   // (P6 J^T)[k][j], (P6 J^T)[k][i]
#pragma unroll
        for (int l = 0; l < 6; ++l) { tj += P6[k][l] * rj[l]; ti += P6[k][l] * ri[l]; }
        cij += ri[k] * tj;
        cji += rj[k] * ti;
    }
    const double cov = 0.5 * (cij + cji);
    // the copied words: p, q (3..9) <- the pose line, v (10..12) <- x_out[17..19], vel_cov (49..57) <- P_out[15..17][15..17] row-major
    const int lc = min(lane, ODOM_WORDS - 1);
    const int v9 = max(lc - 49, 0);
    const double* src = lc < 10 ? pose_out + max(lc - 3, 0) : (lc < 13 ? x_out + 17 + (lc - 10) : P_out + (size_t)(15 + v9 / 3) + (size_t)(15 + v9 % 3) * ld);
    const double copied = *src;
    unsigned long long word;
    if (lane == 0) word = (unsigned long long)seq;
    else if (lane == 1) word = (unsigned long long)(unsigned)img_count | ((unsigned long long)(unsigned)n_clones << 32);
    else if (lane == 2) word = 0ull;
    else if (lane >= 13 && lane < 49) word = (unsigned long long)__double_as_longlong(cov);
    else word = (unsigned long long)__double_as_longlong(copied);
    if (lane < ODOM_WORDS) ring[(size_t)z * ODOM_WORDS + lane] = word;
}
