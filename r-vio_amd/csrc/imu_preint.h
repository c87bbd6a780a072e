// imu_preint.h — the state half of PreIntegrator::propagate's sample loop (PreIntegrator.cc:97-179), stated once for the IMU-rate record kernels:
//   imu_pose_kernel  (imu_pose.hip)          keeps the state behind every sample as a pose record
//   imu_cov_kernel   (imu_cov.hip)           needs the state in front of and behind every sample for Phi, Q and the record's map
// propagate_body (filter_kernels2.hip), which keeps the state behind the last sample, still carries its own text of phases A and B: the same
// expressions, to be replaced by calls of the functions below (ImuTerms / ImuChain / ImuState map onto its Prop3Sample and chain[]).
// The products depend on the three agreeing bit for bit (the last record of the IMU-rate ring IS what propagate leaves; the covariance ring
// shares seq and slot with the pose ring).  tests/test_gpu_imu_bits.py holds all three to the bits of the build these functions were folded out
// of, tests/test_gpu_imu_odometry.py test_last_record_has_the_bits_of_propagate the record kernels to propagate_body.
//
//   imu_sample_terms   what one sample contributes, a function of the sample and the biases alone (parallel over samples): "phase A"
//   imu_chain_step     the serial recursion Rk <- dR Rk, dp, dv, Dt in the reference's order: "phase B"
//   imu_state_behind   pk, vk, gk from the chain's state and the start state (nothing of the chain depends on them)
// and what the two record kernels share around them: the 16-word LDS slot of a sample, the wave fence between their phases, the record's header
// and address.  Register structs are indexed by compile-time constants only (the rule at the head of filter_kernels2.hip).
#pragma once
#include "rvio_dev.h"

// what sample s hands to the chain (16 words) + its bias-free rate, which only the covariance's Phi reads
struct ImuTerms { m33 dR; d3 up, uv; double dt; d3 w; };
// the chain's state behind a step (16 words)
struct ImuChain { m33 Rk; d3 dp, dv; double Dt; };
// the state behind a step: Rk (the chain's), pk, vk, gk
struct ImuState { m33 R; d3 p, v, g; };

// dR, and the two a-dependent vectors through f1..f4 (PreIntegrator.cc:143-167), both nSmallAngle branches
__device__ __forceinline__ ImuTerms imu_sample_terms(const rvio_imu& u, d3 bg, d3 ba, double small_angle) {
    const m33 I = eye33();
    ImuTerms t;
    t.w = sub3(mk3(u.w[0], u.w[1], u.w[2]), bg);
    const d3 w = t.w, a = sub3(mk3(u.a[0], u.a[1], u.a[2]), ba);
    const double dt = u.dt, w1 = nrm3(w);
    const bool small = w1 < small_angle;
    const double wdt = w1 * dt, wdt2 = wdt * wdt;
    double sw, cw;
    sincos(wdt, &sw, &cw);
    const m33 wx = skew33(w), wx2 = mul33(wx, wx);
    double f1, f2, f3, f4;
    if (small) {
        t.dR = add33(sub33(I, scl33(dt, wx)), scl33(dt * dt / 2, wx2));
        f1 = -(dt * dt * dt) / 3; f2 = (dt * dt * dt * dt) / 8; f3 = -(dt * dt) / 2; f4 = (dt * dt * dt) / 6;
    } else {
        const double w2 = w1 * w1, w3 = w2 * w1, w4 = w2 * w2;
        t.dR = add33(sub33(I, scl33(sw / w1, wx)), scl33((1 - cw) / w2, wx2));
        f1 = (wdt * cw - sw) / w3;
        f2 = .5 * (wdt2 - 2 * cw - 2 * wdt * sw + 2) / w4;
        f3 = (cw - 1) / w2;
        f4 = (wdt - sw) / w3;
    }
    t.up = mv33(add33(add33(scl33(.5 * dt * dt, I), scl33(f1, wx)), scl33(f2, wx2)), a);
    t.uv = mv33(add33(add33(scl33(dt, I), scl33(f3, wx)), scl33(f4, wx2)), a);
    t.dt = dt;
    return t;
}

// PreIntegrator.cc:168-174, in that order: dp takes the OLD dv, then both take the NEW Rk
__device__ __forceinline__ void imu_chain_step(ImuChain& c, const ImuTerms& t) {
    c.Dt += t.dt;
    c.Rk = mul33(t.dR, c.Rk);
    const m33 RkT = tr33(c.Rk);
    c.dp = add3(c.dp, scl3(t.dt, c.dv));
    c.dp = add3(c.dp, mv33(RkT, t.up));
    c.dv = add3(c.dv, mv33(RkT, t.uv));
}

// PreIntegrator.cc:175-177 from the start state's (vR, gR): gk re-normalised
__device__ __forceinline__ ImuState imu_state_behind(const ImuChain& c, d3 vR, d3 gR, double nG) {
    ImuState o;
    o.R = c.Rk;
    o.p = add3(sub3(scl3(c.Dt, vR), scl3(.5 * nG * c.Dt * c.Dt, gR)), c.dp);
    o.v = mv33(c.Rk, add3(sub3(vR, scl3(nG * c.Dt, gR)), c.dv));
    o.g = unit3(mv33(c.Rk, gR));
    return o;
}

// ---- the record kernels' LDS slot: 16 words per sample, word-major (word k of sample s at W[k * STRIDE + s]: lane-indexed accesses are
// consecutive 8-byte words, the chain's reads of one sample's words wave-uniform broadcasts).  In front of step s it holds that sample's
// (dR, up, uv, dt); the step overwrites it with (Rk, dp, dv, Dt) behind it.
template <int STRIDE>
__device__ __forceinline__ void imu_slot_put(double* W, int s, const m33& R, d3 a, d3 b, double t) {
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k * STRIDE + s] = R.m[k];
    W[9 * STRIDE + s] = a.x; W[10 * STRIDE + s] = a.y; W[11 * STRIDE + s] = a.z;
    W[12 * STRIDE + s] = b.x; W[13 * STRIDE + s] = b.y; W[14 * STRIDE + s] = b.z;
    W[15 * STRIDE + s] = t;
}
template <int STRIDE>
__device__ __forceinline__ void imu_slot_get(const double* W, int s, m33& R, d3& a, d3& b, double& t) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R.m[k] = W[k * STRIDE + s];
    a = mk3(W[9 * STRIDE + s], W[10 * STRIDE + s], W[11 * STRIDE + s]);
    b = mk3(W[12 * STRIDE + s], W[13 * STRIDE + s], W[14 * STRIDE + s]);
    t = W[15 * STRIDE + s];
}
template <int STRIDE>
__device__ __forceinline__ void imu_put_terms(double* W, int s, const ImuTerms& t) { imu_slot_put<STRIDE>(W, s, t.dR, t.up, t.uv, t.dt); }
template <int STRIDE>
__device__ __forceinline__ ImuTerms imu_get_terms(const double* W, int s) {   // (w is not in the slot)
    ImuTerms t;
    imu_slot_get<STRIDE>(W, s, t.dR, t.up, t.uv, t.dt);
    t.w = mk3(0, 0, 0);
    return t;
}
template <int STRIDE>
__device__ __forceinline__ void imu_put_chain(double* W, int s, const ImuChain& c) { imu_slot_put<STRIDE>(W, s, c.Rk, c.dp, c.dv, c.Dt); }
template <int STRIDE>
__device__ __forceinline__ ImuChain imu_get_chain(const double* W, int s) {
    ImuChain c;
    imu_slot_get<STRIDE>(W, s, c.Rk, c.dp, c.dv, c.Dt);
    return c;
}
// the serial chain over the mc samples whose terms lie in the slots, every lane redundantly (uniform operands, no divergence); lane 0 leaves
// the state behind step s in slot s.  LDS operations of one wave complete in order, so no barrier inside
template <int STRIDE>
__device__ __forceinline__ void imu_chain_chunk(double* W, int mc, int lane, ImuChain& c) {
    for (int s = 0; s < mc; ++s) {
        imu_chain_step(c, imu_get_terms<STRIDE>(W, s));
        if (lane == 0) imu_put_chain<STRIDE>(W, s, c);
    }
}

// Between two phases of ONE wave: its LDS operations complete in program order; the fence keeps the compiler from moving them across the boundary
__device__ __forceinline__ void imu_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the record of sample j (of m) of instance z, WORDS 8-byte words long.  predict (cap == 0): at out[z * out_stride + j], seq 0; ring
// (cap > 0): seq = seq0 + j, slot (seq - 1) % cap of ring[cap][batch] — of a batch longer than the ring only the last cap records are stored
// (two records of one launch never share a slot).  Both rings use this rule, so a covariance record and its pose record share seq and slot.
__device__ __forceinline__ bool imu_record_stored(int j, int m, int cap) { return cap == 0 || j >= m - cap; }
// writes words 0 (seq) and 1 (img_count | index << 32), returns the record
template <int WORDS>
__device__ __forceinline__ unsigned long long* imu_record(unsigned long long* out, int z, int j, int batch, long long out_stride, long long seq0, int cap, int img_count) {
    const long long seq = cap ? seq0 + j : 0;
    const size_t rec = cap ? (size_t)((seq - 1) % cap) * (size_t)batch + (size_t)z : (size_t)z * (size_t)out_stride + (size_t)j;
    unsigned long long* o = out + rec * WORDS;
    o[0] = (unsigned long long)seq;
    o[1] = (unsigned long long)(unsigned)img_count | ((unsigned long long)(unsigned)j << 32);
    return o;
}
__device__ __forceinline__ unsigned long long imu_word(double v) { return (unsigned long long)__double_as_longlong(v); }
