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
//   A  lane s <-> sample s: imu_sample_terms (imu_preint.h) into the sample's LDS slot
//   B  the serial chain over the chunk, every lane redundantly (imu_chain_chunk).  Its state carries across chunks in registers.  pk and vk are
//      functions of the chain's state and of the start state only — nothing of the chain depends on them —, so they are formed in phase C, in parallel
//   C  lane s <-> record s: imu_state_behind, RotToQuat(Rk), QuatMul with qG, R(qG)^T (pk - pG) with the device functions augcomp_kernel2 uses
// Sample s's terms reach the chain through LDS: imu_preint.h's 16-word slot at stride 64 = 8 KB per wave.  Step s overwrites ITS sample's slot
// with the state behind that step (one lane stores).  Cross-lane reads (v_readlane) instead would be 32 scalar-indexed reads per step on the
// chain's own issue port plus 32 selects per step to leave "lane s keeps step s" behind — more instructions on the one wave's serial path than
// 16 broadcast loads and 16 stores that the LDS pipeline takes off it.
#pragma once
#include "imu_preint.h"
#define IMUP_WORDS 13   // sizeof(rvio_imu_pose) / 8

// out, out_stride, seq0, cap: imu_record's (imu_preint.h).  x / imu: instance 0's; instance z lies z * bs / z * imu_bs bytes behind (imu_bs = 0:
// one shared batch).
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
    ImuChain c = {q2r(ldq(x + 10)), mk3(0, 0, 0), mk3(0, 0, 0), 0.0};
    for (int s0 = 0; s0 < m; s0 += 64) {
        const int mc = (m - s0 < 64) ? (m - s0) : 64;
        // ---- A
        double t_s = 0.0;
        if (lane < mc) {
            const rvio_imu u = imu[s0 + lane];
            imu_put_terms<64>(W, lane, imu_sample_terms(u, bg, ba, small_angle));
            t_s = u.t;
        }
        imu_wave_fence();
        // ---- B
        imu_chain_chunk<64>(W, mc, lane, c);
        imu_wave_fence();
        // ---- C
        const int j = s0 + lane;
        if (lane < mc && imu_record_stored(j, m, cap)) {
            const ImuChain cs = imu_get_chain<64>(W, lane);
            const ImuState b = imu_state_behind(cs, vR, gR, nG);
            const q4 qkG = qmul(r2q(cs.Rk), qG);
            const d3 pGk = mv33(tr33(q2r(qG)), sub3(b.p, pG));   // pose line (System.cc:371-374)
            unsigned long long* o = imu_record<IMUP_WORDS>(out, z, j, batch, out_stride, seq0, cap, img_count);
            o[2] = imu_word(t_s);
            o[3] = imu_word(pGk.x); o[4] = imu_word(pGk.y); o[5] = imu_word(pGk.z);
            o[6] = imu_word(qkG.x); o[7] = imu_word(qkG.y); o[8] = imu_word(qkG.z); o[9] = imu_word(qkG.w);
            o[10] = imu_word(b.v.x); o[11] = imu_word(b.v.y); o[12] = imu_word(b.v.z);
        }
        imu_wave_fence();   // (the next chunk's phase A rewrites the slots phase C has read: same wave, program order)
    }
}
