// imu_cov.hip — the covariance of IMU-rate odometry (rvio_imu_cov of include/rvio_hip.h): the pose_cov / vel_cov an rvio_odom record would
// carry if an image arrived right behind IMU sample j and that frame ran no update, for EVERY sample of a batch.  PreIntegrator::propagate
// advances the 24 x 24 head of P once per sample (PreIntegrator.cc:123-142) and keeps the last; this kernel keeps, behind every step, what
// composition (System.cc:325-365) and odom_kernel's map make of it.  It writes covariance records only: the paired pose records are
// imu_pose_kernel's.
//
//   P11 <- Phi_s P11 Phi_s^T + Q_s,   Phi_s = I + dt F_s,   Q_s = (dt G_s) Sigma G_s^T        F_s, G_s from (Rk, vk, gk) IN FRONT of step s
//   P6_j = Vk_j[0..5][:] P11_j Vk_j[0..5][:]^T                                                  Vk_j from (Rk_j, pk_j, pG) BEHIND step j
//   pose_cov_j = (C + C^T) / 2,  C = J_j P6_j J_j^T,  J_j = odom.hip's map at (qjG, pjG = Rk_j (pG - pk_j));   vel_cov_j = sym(P11_j)[15..17][15..17]
// No clone cross-terms: the marginal of the head does not depend on them.
//
// Launched by rvio_hip_predict_cov[_dev] and, when the covariance ring is on (rvio_hip_set_imu_odometry_cov), right next to imu_pose_kernel.
// It reads x[0..25], the 24 x 24 head of P (column-major, leading dimension ld) and the IMU batch.
//
// Geometry (launch_plan.h LP_IMUC_*): one wave per instance, one instance per 64-thread workgroup, no block-wide barrier.  Per chunk of up to
// LP_IMUC_CHUNK samples the wave runs
//   A  lane s <-> sample s: imu_sample_terms (imu_preint.h) into words 0..15 of the sample's slot
//   B  the serial STATE chain, every lane redundantly (imu_chain_chunk).  Step s leaves (Rk, dp, dv, Dt) behind it in those words
//   C  lane s <-> sample s: (Rk, vk, gk) in front of the step (slot s - 1; the chunk's first sample: carried in registers, at s = 0 the raw
//      x[10..13], x[17..19], x[7..9]) -> the six distinct non-zero 3 x 3 blocks of dt F_s, dt, and the block of Q_s in rows / columns 9..17, into the
//      slot; (Rk_s, pk_s) behind the step stay in the lane's registers for phase E
//   D  the serial COVARIANCE chain.  Lane c < 24 keeps COLUMN c of P11 in 24 registers, across steps and chunks.  F is non-zero in rows 9..17
//      only, so T = Phi P11 changes rows 9..17 only and is column-local: 81 FMAs per lane on the step's blocks, which every lane reads from LDS
//      at a wave-uniform address (one broadcast each).  T Phi^T changes columns 9..17 only; with P11 symmetric P11 Phi^T = (Phi P11)^T, so
//      column c of it, 9 <= c < 18, is ROW c of T — nine words per lane through LDS and back — and Phi applied to that column (the same 81
//      FMAs) plus Q's column finishes it.  Lanes 18..23 add the bias noise to their diagonal entry.  What the record needs — the 12 x 12
//      block on rows / columns {0-5, 9-14} and the 3 x 3 velocity block — goes over the sample's blocks, which are spent.
//      (The reference forms Phi P11 Phi^T without using the symmetry; the two agree to rounding on the symmetric P11 every stage of the filter
//      leaves, which is the only kind the handle holds.)
//   E  lane s <-> record s: Vk and J as 3 x 3 blocks (30 block products; register arrays under compile-time indices only, the rule at the head of
//      filter_kernels2.hip), C_ij and C_ji formed separately and added in either order — the same two numbers, hence the same bits.
// LDS per wave: 169 words x LP_IMUC_CHUNK samples — imu_preint.h's 16-word slot at stride LP_IMUC_CHUNK, and this kernel's own words behind
// it in the same word-major layout —, + the nine rows of T (216).  The phases of one wave are ordered by imu_wave_fence.
#pragma once
#include "imu_preint.h"
#define IMUC_WORDS 47   // sizeof(rvio_imu_cov) / 8
#define IMUC_SLOT(W, k, s) (W)[(k) * LP_IMUC_CHUNK + (s)]   // this kernel's words of sample s, k >= IMUC_PHI
#define IMUC_PHI 16                  // dt F's blocks, row-major 3 x 3 each: A1 = -dt [w x], B1 = -dt Rk^T [v x], B2 = dt Rk^T, C1 = -dt g Rk, C2 = -dt g [gk x], C3 = -dt [v x]
#define IMUC_DT (IMUC_PHI + 54)
#define IMUC_Q (IMUC_PHI + 55)       // 9 x 9, row-major: Q rows / columns 9..17
#define IMUC_OUT IMUC_PHI            // behind the step: 144 words of the 12 x 12 block, row-major, + 9 of the velocity block
static_assert(IMUC_Q + 81 <= LP_IMUC_SLOT_WORDS && IMUC_OUT + 153 == LP_IMUC_SLOT_WORDS, "launch_plan.h: imu_cov_kernel's slot");

// the state behind the step whose chain state lies in slot s
__device__ __forceinline__ ImuState imuc_state(const double* W, int s, d3 vR, d3 gR, double nG) {
    return imu_state_behind(imu_get_chain<LP_IMUC_CHUNK>(W, s), vR, gR, nG);
}
struct ImucPhi { m33 A1, B1, B2, C1, C2, C3; double dt; };
__device__ __forceinline__ m33 imuc_ld33(const double* W, int base, int s) {
    m33 B;
#pragma unroll
    for (int k = 0; k < 9; ++k) B.m[k] = IMUC_SLOT(W, base + k, s);
    return B;
}
// rows 9..17 of Phi V for a column V of 24 entries, k ascending within a row (PreIntegrator.cc:123-135: Phi = I + dt F)
__device__ __forceinline__ void imuc_apply(const ImucPhi& F, const double (&V)[24], double (&T)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double a = V[9 + i], b = V[12 + i], c = V[15 + i];
#pragma unroll
        for (int j = 0; j < 3; ++j) { a += F.A1.m[3 * i + j] * V[9 + j]; b += F.B1.m[3 * i + j] * V[9 + j]; c += F.C1.m[3 * i + j] * V[6 + j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { b += F.B2.m[3 * i + j] * V[15 + j]; c += F.C2.m[3 * i + j] * V[9 + j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) c += F.A1.m[3 * i + j] * V[15 + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) c += F.C3.m[3 * i + j] * V[18 + j];
        a -= F.dt * V[18 + i];
        c -= F.dt * V[21 + i];
        T[i] = a; T[3 + i] = b; T[6 + i] = c;
    }
}
// a 3 x 3 block into a row-major matrix of `cols` columns that starts at word `base` of sample s's slot
__device__ __forceinline__ void imuc_put33(double* W, int base, int cols, int r0, int c0, const m33& B, int s) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) IMUC_SLOT(W, base + (r0 + i) * cols + c0 + j, s) = B.m[3 * i + j];
}
// block (a, b) of the 12 x 12 output block of sample s
__device__ __forceinline__ m33 imuc_blk(const double* W, int a, int b, int s) {
    m33 B;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B.m[3 * i + j] = IMUC_SLOT(W, IMUC_OUT + (3 * a + i) * 12 + 3 * b + j, s);
    return B;
}
__device__ __forceinline__ m33 imuc_mulT(const m33& A, const m33& B) { return mul33(A, tr33(B)); }   // A B^T

// out, out_stride, seq0, cap: imu_record's (imu_preint.h).  x / P / imu: instance 0's; instance z lies z * bs / z * imu_bs bytes behind
// (imu_bs = 0: one shared batch).
__global__ __launch_bounds__(LP_IMUC_T) void imu_cov_kernel(double small_angle, double nG, double sg2, double swg2, double sa2, double swa2, int batch,
                                                            const double* __restrict__ x, const double* __restrict__ P, int ld, size_t bs,
                                                            const rvio_imu* __restrict__ imu, size_t imu_bs, int m,
                                                            unsigned long long* __restrict__ out, long long out_stride, long long seq0, int cap,
                                                            int img_count) {
    extern __shared__ __align__(16) double imuc_dyn[];
    const int lane = threadIdx.x & 63;
    const int z = (int)blockIdx.x;
    if (z >= batch) return;
    double* W = imuc_dyn;
    double* Tl = W + LP_IMUC_SLOT_WORDS * LP_IMUC_CHUNK;   // rows 9..17 of Phi P11, row-major 9 x 24
    x = zoffi(x, bs, z); P = zoffi(P, bs, z); imu = zoffi(imu, imu_bs, z);
    const q4 qG = ldq(x);
    const d3 pG = ld3(x + 4);
    const d3 bg = ld3(x + 20), ba = ld3(x + 23);
    const d3 gR = ld3(x + 7), vR = ld3(x + 17);
    const m33 I = eye33();
    const m33 RG = q2r(qG);
    // the state chain's registers, and the state in front of the chunk's first step
    ImuChain c = {q2r(ldq(x + 10)), mk3(0, 0, 0), mk3(0, 0, 0), 0.0};
    m33 Rf = c.Rk;
    d3 vf = vR, gf = gR;
    // column cc of P11 (the lanes beyond 23 carry column 23 along and store nothing)
    const int cc = min(lane, 23), ci = min(max(cc - 9, 0), 8);
    const bool col = lane < 24, mid = cc >= 9 && cc < 18;
    double Pc[24];
#pragma unroll
    for (int r = 0; r < 24; ++r) Pc[r] = P[(size_t)r + (size_t)cc * ld];
    for (int s0 = 0; s0 < m; s0 += LP_IMUC_CHUNK) {
        const int mc = (m - s0 < LP_IMUC_CHUNK) ? (m - s0) : LP_IMUC_CHUNK;
        const bool mine = lane < mc;
        const int sl = mine ? lane : 0;   // (idle lanes read sample 0's words along and drop the results: every LDS address stays inside the slab)
        // ---- A
        d3 w = mk3(0, 0, 0);
        double dt_s = 0.0;
        if (mine) {
            const ImuTerms t = imu_sample_terms(imu[s0 + lane], bg, ba, small_angle);
            imu_put_terms<LP_IMUC_CHUNK>(W, lane, t);
            w = t.w; dt_s = t.dt;
        }
        imu_wave_fence();
        // ---- B
        imu_chain_chunk<LP_IMUC_CHUNK>(W, mc, lane, c);
        imu_wave_fence();
        // ---- C
        const ImuState bh = imuc_state(W, sl, vR, gR, nG);                      // behind this lane's step
        const ImuState pv = imuc_state(W, sl > 0 ? sl - 1 : 0, vR, gR, nG);     // behind the step before it
        const ImuState last = imuc_state(W, mc - 1, vR, gR, nG);                // behind the chunk (uniform)
        {
            const bool first = sl == 0;
            m33 Rs;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rs.m[k] = first ? Rf.m[k] : pv.R.m[k];
            const d3 vs = first ? vf : pv.v, gs = first ? gf : pv.g;
            const double dt = dt_s;
            const m33 wx = skew33(w), vx = skew33(vs), RsT = tr33(Rs);
            if (mine) {
                // dt F (PreIntegrator.cc:123-133) and Q = (dt G) Sigma G^T on rows / columns 9..17 (:136-141): G[9][0] = -I, G[15][0] = -[v x], G[15][6] = -I
                imuc_put33(W, IMUC_PHI, 3, 0, 0, scl33(dt, scl33(-1.0, wx)), lane);
                imuc_put33(W, IMUC_PHI + 9, 3, 0, 0, scl33(dt, mul33(scl33(-1.0, RsT), vx)), lane);
                imuc_put33(W, IMUC_PHI + 18, 3, 0, 0, scl33(dt, RsT), lane);
                imuc_put33(W, IMUC_PHI + 27, 3, 0, 0, scl33(dt, scl33(-nG, Rs)), lane);
                imuc_put33(W, IMUC_PHI + 36, 3, 0, 0, scl33(dt, scl33(-nG, skew33(gs))), lane);
                imuc_put33(W, IMUC_PHI + 45, 3, 0, 0, scl33(dt, scl33(-1.0, vx)), lane);
                IMUC_SLOT(W, IMUC_DT, lane) = dt;
                const m33 Z = scl33(0.0, I), qvx = scl33(dt * sg2, vx);
                imuc_put33(W, IMUC_Q, 9, 0, 0, scl33(dt * sg2, I), lane); imuc_put33(W, IMUC_Q, 9, 0, 3, Z, lane); imuc_put33(W, IMUC_Q, 9, 0, 6, tr33(qvx), lane);
                imuc_put33(W, IMUC_Q, 9, 3, 0, Z, lane); imuc_put33(W, IMUC_Q, 9, 3, 3, Z, lane); imuc_put33(W, IMUC_Q, 9, 3, 6, Z, lane);
                imuc_put33(W, IMUC_Q, 9, 6, 0, qvx, lane); imuc_put33(W, IMUC_Q, 9, 6, 3, Z, lane);
                imuc_put33(W, IMUC_Q, 9, 6, 6, add33(imuc_mulT(qvx, vx), scl33(dt * sa2, I)), lane);
            }
        }
        Rf = last.R; vf = last.v; gf = last.g;
        imu_wave_fence();
        // ---- D
        for (int s = 0; s < mc; ++s) {
            ImucPhi F;
            F.A1 = imuc_ld33(W, IMUC_PHI, s); F.B1 = imuc_ld33(W, IMUC_PHI + 9, s); F.B2 = imuc_ld33(W, IMUC_PHI + 18, s);
            F.C1 = imuc_ld33(W, IMUC_PHI + 27, s); F.C2 = imuc_ld33(W, IMUC_PHI + 36, s); F.C3 = imuc_ld33(W, IMUC_PHI + 45, s);
            F.dt = IMUC_SLOT(W, IMUC_DT, s);
            // T = Phi P11: rows 9..17 of this lane's column
            double Tc[9];
            imuc_apply(F, Pc, Tc);
            if (col) {
#pragma unroll
                for (int i = 0; i < 9; ++i) Tl[i * 24 + lane] = Tc[i];
            }
            imu_wave_fence();
            // columns 9..17: P11 Phi^T's column is T's row; Phi on it, plus Q's column
            double V[24], T2[9];
#pragma unroll
            for (int r = 0; r < 24; ++r) V[r] = Tl[ci * 24 + r];
            imuc_apply(F, V, T2);
#pragma unroll
            for (int i = 0; i < 9; ++i) T2[i] += IMUC_SLOT(W, IMUC_Q + i * 9 + ci, s);
#pragma unroll
            for (int r = 0; r < 24; ++r) {
                if (r >= 9 && r < 18) Pc[r] = mid ? T2[r - 9] : Tc[r - 9];
                else Pc[r] = mid ? V[r] : Pc[r];
            }
            // the process noise of the biases: G[18][3] = G[21][9] = I
#pragma unroll
            for (int r = 18; r < 24; ++r) Pc[r] += (cc == r) ? F.dt * (r < 21 ? swg2 : swa2) : 0.0;
            imu_wave_fence();   // (the blocks and T's rows are read: the record's words may go over the first, the next step's T over the second)
            // what the record needs, over the sample's blocks
            const int cb = cc < 6 ? cc : cc - 3;
            if (col && (cc < 6 || (cc >= 9 && cc < 15))) {
#pragma unroll
                for (int a = 0; a < 12; ++a) IMUC_SLOT(W, IMUC_OUT + a * 12 + cb, s) = Pc[a < 6 ? a : a + 3];
            }
            if (lane >= 15 && lane < 18) {
#pragma unroll
                for (int i = 0; i < 3; ++i) IMUC_SLOT(W, IMUC_OUT + 144 + i * 3 + (lane - 15), s) = Pc[15 + i];
            }
        }
        imu_wave_fence();
        // ---- E
        const int j = s0 + lane;
        if (mine && (cap == 0 || j >= m - cap)) {
            const m33 Rj = bh.R;
            const d3 pjG = mv33(Rj, sub3(pG, bh.p));            // System.cc:340 with pk_j for pk
            const m33 S = skew33(pjG);
            const m33 R = mul33(Rj, RG);                         // R(qjG) = R(qk_j) R(qG)
            const m33 RT = tr33(R), A = mul33(RT, S);            // J = [A, -R^T; R^T, 0]  (odom.hip)
            // W = Vk[0..5] P12 (blocks: 0 rot G, 1 pos G, 2 rot k, 3 pos k): W0b = Rk A0b + A2b, W1b = Rk (A1b - A3b) + [pjG x] A2b
            m33 W0[4], W1[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const m33 A2 = imuc_blk(W, 2, b, lane);
                W0[b] = add33(mul33(Rj, imuc_blk(W, 0, b, lane)), A2);
                W1[b] = add33(mul33(Rj, sub33(imuc_blk(W, 1, b, lane), imuc_blk(W, 3, b, lane))), mul33(S, A2));
            }
            // P6 = W Vk[0..5]^T
            const m33 P00 = add33(imuc_mulT(W0[0], Rj), W0[2]), P01 = add33(imuc_mulT(sub33(W0[1], W0[3]), Rj), imuc_mulT(W0[2], S));
            const m33 P10 = add33(imuc_mulT(W1[0], Rj), W1[2]), P11 = add33(imuc_mulT(sub33(W1[1], W1[3]), Rj), imuc_mulT(W1[2], S));
            // X = J P6, C = X J^T
            const m33 X00 = sub33(mul33(A, P00), mul33(RT, P10)), X01 = sub33(mul33(A, P01), mul33(RT, P11));
            const m33 X10 = mul33(RT, P00), X11 = mul33(RT, P01);
            const m33 C00 = sub33(imuc_mulT(X00, A), imuc_mulT(X01, RT)), C01 = imuc_mulT(X00, RT);
            const m33 C10 = sub33(imuc_mulT(X10, A), imuc_mulT(X11, RT)), C11 = imuc_mulT(X10, RT);
            // (imu_record's rule and imu_record_stored's above, written out: through the helpers this kernel allocates 2 to 8 registers more
            // than the 500 it has, and it has none to spare)
            const long long seq = cap ? seq0 + j : 0;
            const size_t rec = cap ? (size_t)((seq - 1) % cap) * (size_t)batch + (size_t)z : (size_t)z * (size_t)out_stride + (size_t)j;
            unsigned long long* o = out + rec * IMUC_WORDS;
            o[0] = (unsigned long long)seq;
            o[1] = (unsigned long long)(unsigned)img_count | ((unsigned long long)(unsigned)j << 32);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    // (a, b) of the four blocks; the mirror entry adds the same two numbers in the other order
                    o[2 + a * 6 + b] = imu_word(0.5 * (C00.m[3 * a + b] + C00.m[3 * b + a]));
                    o[2 + a * 6 + 3 + b] = imu_word(0.5 * (C01.m[3 * a + b] + C10.m[3 * b + a]));
                    o[2 + (3 + a) * 6 + b] = imu_word(0.5 * (C10.m[3 * a + b] + C01.m[3 * b + a]));
                    o[2 + (3 + a) * 6 + 3 + b] = imu_word(0.5 * (C11.m[3 * a + b] + C11.m[3 * b + a]));
                }
#pragma unroll
            for (int k = 0; k < 9; ++k) {   // sym(P11)[15..17][15..17]
                const int kt = 3 * (k % 3) + k / 3;
                o[38 + k] = imu_word(0.5 * (IMUC_SLOT(W, IMUC_OUT + 144 + k, lane) + IMUC_SLOT(W, IMUC_OUT + 144 + kt, lane)));
            }
        }
        // (the next chunk's phase A rewrites the slots phase E has read: same wave, program order)
        imu_wave_fence();
    }
}
