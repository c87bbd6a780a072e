// landmark_cov.hip — the 3 x 3 covariance of every point of the landmark cloud (rvio_landmark_cov of include/rvio_hip.h).
//
// Launched directly behind landmark_kernel (update_global_dev) when enabled (rvio_hip_set_landmark_cov).  It reads feat[] and count as
// landmark_kernel left them — order and membership are the cloud's by construction — and, like it, the hand-over table's types and lengths,
// (phi, psi, rho), the state the update read (xk1k) and the per-instance calibration; beside them the covariance the update read (P of the same
// buffer, untouched until augcomp_kernel2 rewrites it).  It writes its records, nothing else.
//
// The quantity.  theta = (phi, psi, rho) is no state: it is the least-squares solution of all L observations of the track given the clones, so to
// first order dtheta = -A (Hx dx + n), A = N^-1 Hf^T, N = Hf^T Hf, n ~ sigma^2 I (sigma: DevCfg::sigma_im, the update's own).  With the chain
//   X_0 = R_ic e / rho + t_ic,  X_{i+1} = R_i (X_i - p_i),  RI_{i+1} = R_i RI_i,  tI_{i+1} = R_i (tI_i - p_i)      (i = 0 .. nPh - 1, nPh = L - 1)
// over the track's clones (type '1': the newest nPh, type '2': the oldest), X_i is the point in the IMU frame of image i and p_r = X_nPh:
//   Hp_i = d(h / h_z) / dh at h = rho R_ci (X_i - t_ic)
//   Hf_i = Hp_i [R_ci RI_i R_ic Jang | R_ci ((RI_i - I) t_ic + tI_i)]                            (2 x 3; before the nullspace projection, ALL L)
//   Hx_i[clone j < i] = rho Hp_i R_ci RI_i RI_{j+1}^T E_j,   E_j = [ [X_{j+1} x] | -R_j ]        (2 x 6; never stored)
//   Jth = RI_nPh R_ic [Jang / rho | -e / rho^2],   Jx[clone j] = RI_nPh RI_{j+1}^T E_j
//   M[clone j] = Jx_j - Jth A Hx_j = (RI_nPh - sum_{i > j} Jth N^-1 Hf_i^T rho Hp_i R_ci RI_i) RI_{j+1}^T E_j
//   cov_r = sigma^2 Jth N^-1 Jth^T + M P_span M^T
//   p_w = R_G^T (p_r - pG) at the SAME prior state,  M_w = R_G^T [ -[(p_r - pG) x] | -I | M ]  over columns 0 .. 5 and the span
//   cov_w = sigma^2 (R_G^T Jth) N^-1 (R_G^T Jth)^T + M_w P M_w^T,   rho_sigma^2 = sigma^2 (N^-1)_22 + a P_span a^T,  a = row 2 of A Hx
// in the error convention of P (R_true ~ (I - [dth x]) R, positions additive).  The translation column of Hf is formed without t_ci, so that a
// track whose clones do not move gives an exactly zero column.
//
// Grid (cloud slots, 1, instances), ONE workgroup of LP_LMC_T = 256 threads per (instance, slot), FP64, plain C++, static LDS only (one array
// of LP_LMC_LDS_DOUBLES doubles), no atomics, no scratch.  A workgroup whose slot is at or beyond the cloud's count returns at once.
//   1  thread i < nPh: R_i, p_i of the track's clones; threads 0 / 64 / 128 then run the three recurrences X, tI, RI (one wave each)
//   2  thread i < L: Hp_i, Hf_i and W_i = rho Hp_i R_ci; threads 0 .. 5 sum the six entries of N over i = 0 .. L - 1 in that order; thread 0
//      factors N (3 x 3 Cholesky; a pivot <= LP_LMC_PIVOT_EPS N_kk: status 1, NaN covariances, the points still filled), forms N^-1,
//      Y = Jth N^-1 and the three noise terms
//   3  thread i < L: Q_i = [Y; (N^-1)_2] Hf_i^T W_i RI_i (4 x 3); thread j < nPh: S_j = (sum_{i = j+1 .. nPh} Q_i) RI_{j+1}^T in rising i, then
//      the seven rows of its six columns: M, R_G^T M and the rho row; thread 64 the head columns.  rows[entry][7] in LDS, the Jacobians not
//   4  T = P_nz rows^T: thread <-> entry of the compacted set 0 .. 5, 24 + 6 c0 .. 24 + 6 (c0 + nPh) - 1 (at most 192: one pass), seven
//      accumulators; P is symmetric and column-major, so consecutive threads read consecutive doubles of one column per load.  Every column of
//      P outside that set is never read
//   5  C = rows T: thread (g, entry) with entry one of the 9 + 9 + 1 and g one of LP_LMC_GROUPS = 13 groups taking e = g, g + 13, ... in rising
//      order, both orders (ij, ji) of its entry; thread entry adds the thirteen shares in the order 0 .. 12, halves the sum of the two orders and
//      adds the noise term, itself the half sum of its two orders: cov_r and cov_w are symmetric bit for bit, the same bits every run
//   6  the 28 words of the record from LDS: one coalesced store
// p_r of the record is the cloud's own value, copied (landmark_kernel carries the chain as quaternions in the reference's order; this kernel
// carries rotation matrices: the same to rounding, and the Jacobians use this kernel's).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): 108 VGPRs, 0 AGPRs, 104 SGPRs, no scratch, no spills, static LDS 40 488 B
// (= 8 LP_LMC_LDS_DOUBLES: four workgroups per CU), occupancy 4 waves / SIMD; grid (ceil(n_features / 2), 1, instances) x 256 threads.
struct LmcOut { unsigned long long* rec; size_t stride; };   // records of instance 0; instance z lies z * stride records behind

__device__ __forceinline__ int lmc_col(int e, int cbase) { return e < 6 ? e : cbase + e - 6; }   // column of P of entry e of the compacted set
__device__ __forceinline__ void lmc_st33(double* p, const m33& A) {
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = A.m[k];
}

__global__ __launch_bounds__(LP_LMC_T) void landmark_cov_kernel(DevCfg cfg, int n, int ld, const double* __restrict__ xk1k, const double* __restrict__ P,
                                                               const unsigned char* types, const int* lens, const double* pfinv, size_t bs,
                                                               BatchIn bin, LmOut lm, const CamCal* __restrict__ cal, LmcOut out) {
    static_assert(LP_LMC_T == 256 && LP_LMC_LMAX <= 64 && LP_LMC_NZ <= LP_LMC_T, "four waves; one lane per observation, one thread per non-zero column");
    __shared__ __align__(16) double sm[LP_LMC_LDS_DOUBLES];
    double* const Rs = sm;                                   // [nPh][9]
    double* const ps = Rs + LP_FIXP_NMAX * 9;                // [nPh][3]
    double* const RIs = ps + LP_FIXP_NMAX * 3;               // [L][9]
    double* const Xs = RIs + LP_LMC_LMAX * 9;                // [L][3]
    double* const tIs = Xs + LP_LMC_LMAX * 3;                // [L][3]
    double* const Hfs = tIs + LP_LMC_LMAX * 3;               // [L][2][3]
    double* const Ws = Hfs + LP_LMC_LMAX * 6;                // [L][2][3]
    double* const Qs = Ws + LP_LMC_LMAX * 6;                 // [L][4][3]
    double* const rows = Qs + LP_LMC_LMAX * 12;              // [entry][7]
    double* const Ts = rows + LP_LMC_ROWS * LP_LMC_NZ;       // [entry][7]
    double* const part = Ts + LP_LMC_ROWS * LP_LMC_NZ;       // [group * ENTS + entry][2]
    double* const misc = part + LP_LMC_GROUPS * LP_LMC_ENTS * 2;   // 96: see the offsets below
    unsigned long long* const rec = (unsigned long long*)(misc + 96);
    double* const m_e = misc;          // e (3)
    double* const m_J = misc + 3;      // Jang (3 x 2)
    double* const m_N = misc + 9;      // N (3 x 3)
    double* const m_G = misc + 18;     // [Y; (N^-1)_2] (4 x 3)
    double* const m_noise = misc + 30; // the noise term of every entry (19)
    double* const m_RG = misc + 49;    // R_G (3 x 3)
    double* const m_st = misc + 58;    // status (as a double: 0 / 1)

    const int z = (int)blockIdx.z, slot = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int cnt = min(max(*zoffi(lm.count, lm.bs, z), 0), cfg.Fu);
    if (slot >= cnt) return;
    xk1k = zoffi(xk1k, bs, z); P = zoffi(P, bs, z); pfinv = zoffi(pfinv, bs, z);
    types = zoffi(types, bin.types, z); lens = zoffi(lens, bin.len, z);
    unsigned long long* o = out.rec + ((size_t)z * out.stride + (size_t)slot) * LP_LMC_WORDS;
    const int f = zoffi(lm.feat, lm.bs, z)[slot];
    const double* prc = zoffi(lm.p_r, lm.bs, z) + 3 * slot;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int L = 0, nPh = 0;
    unsigned char type = 0;
    if (f >= 0 && f < cfg.Fu) { type = types[f]; L = lens[f]; nPh = L - 1; }
    if (!(nPh >= 1 && nPh <= n && n <= LP_FIXP_NMAX && (type == '1' || type == '2'))) {
        // (landmark_kernel admits no such member: the reads below stay inside the state whatever the buffers hold)
        if (tid < LP_LMC_WORDS) {
            unsigned long long w = (unsigned long long)__double_as_longlong(qnan);
            if (tid == 0) w = (unsigned long long)(unsigned)f | ((unsigned long long)(unsigned)L << 32);
            if (tid == 1) w = 1ull;
            o[tid] = w;
        }
        return;
    }
    const int c0 = type == '1' ? n - nPh : 0;            // the first clone of the track
    const int nz = 6 + 6 * nPh, cbase = 24 + 6 * c0;
    const double phi = pfinv[3 * f], psi = pfinv[3 * f + 1], rho = pfinv[3 * f + 2];
    const CamCal cam = cam_of(cfg, cal, z);
    const m33 Ric = ldm33(cam.Ric), Rci = ldm33(cam.Rci);
    const d3 tic = ld3(cam.tic);

    // ---- 1  the chain
    if (tid < nPh) {
        const double* c = xk1k + 26 + 7 * (c0 + tid);
        lmc_st33(Rs + 9 * tid, q2r(ldq(c)));
        st3(ps + 3 * tid, ld3(c + 4));
    }
    if (tid == 192) {
        const double cp = cos(phi), sp = sin(phi), cs = cos(psi), ss = sin(psi);
        m_e[0] = cp * ss; m_e[1] = sp; m_e[2] = cp * cs;
        m_J[0] = -sp * ss; m_J[1] = cp * cs; m_J[2] = cp; m_J[3] = 0.0; m_J[4] = -sp * cs; m_J[5] = -cp * ss;
        lmc_st33(m_RG, q2r(ldq(xk1k)));
    }
    __syncthreads();
    if (tid == 0) {
        d3 X = add3(mv33(Ric, scl3(1 / rho, ld3(m_e))), tic);
        st3(Xs, X);
        for (int i = 0; i < nPh; ++i) { X = mv33(ldm33(Rs + 9 * i), sub3(X, ld3(ps + 3 * i))); st3(Xs + 3 * (i + 1), X); }
    } else if (tid == 64) {
        d3 t = mk3(0.0, 0.0, 0.0);
        st3(tIs, t);
        for (int i = 0; i < nPh; ++i) { t = mv33(ldm33(Rs + 9 * i), sub3(t, ld3(ps + 3 * i))); st3(tIs + 3 * (i + 1), t); }
    } else if (tid == 128) {
        m33 A = eye33();
        lmc_st33(RIs, A);
        for (int i = 0; i < nPh; ++i) { A = mul33(ldm33(Rs + 9 * i), A); lmc_st33(RIs + 9 * (i + 1), A); }
    }
    __syncthreads();

    // ---- 2  Hf_i, W_i; N; its factor, Y and the noise terms
    if (tid < L) {
        const m33 RI = ldm33(RIs + 9 * tid);
        const d3 pc = mv33(Rci, sub3(ld3(Xs + 3 * tid), tic));
        const d3 h = scl3(rho, pc);
        const double iz = 1 / h.z, hx = -h.x / (h.z * h.z), hy = -h.y / (h.z * h.z);     // Hp = [iz 0 hx; 0 iz hy]
        const m33 Rc = mul33(mul33(Rci, RI), Ric);
        const d3 tc = mv33(Rci, add3(mv33(sub33(RI, eye33()), tic), ld3(tIs + 3 * tid)));
        double* hf = Hfs + 6 * tid;
        double* w = Ws + 6 * tid;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const d3 v = mk3(Rc.m[0] * m_J[b] + Rc.m[1] * m_J[2 + b] + Rc.m[2] * m_J[4 + b], Rc.m[3] * m_J[b] + Rc.m[4] * m_J[2 + b] + Rc.m[5] * m_J[4 + b],
                             Rc.m[6] * m_J[b] + Rc.m[7] * m_J[2 + b] + Rc.m[8] * m_J[4 + b]);     // column b of R_c Jang
            hf[b] = iz * v.x + hx * v.z;
            hf[3 + b] = iz * v.y + hy * v.z;
        }
        hf[2] = iz * tc.x + hx * tc.z;
        hf[5] = iz * tc.y + hy * tc.z;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            w[c] = rho * (iz * Rci.m[c] + hx * Rci.m[6 + c]);
            w[3 + c] = rho * (iz * Rci.m[3 + c] + hy * Rci.m[6 + c]);
        }
    }
    __syncthreads();
    if (tid < 6) {
        const int a = tid < 3 ? 0 : (tid < 5 ? 1 : 2), b = tid < 3 ? tid : (tid < 5 ? tid - 2 : 2);
        double s = 0.0;
        for (int i = 0; i < L; ++i) s += Hfs[6 * i + a] * Hfs[6 * i + b] + Hfs[6 * i + 3 + a] * Hfs[6 * i + 3 + b];
        m_N[3 * a + b] = s; m_N[3 * b + a] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const double sig2 = cfg.sigma_im * cfg.sigma_im;
        double l00 = 0, l10 = 0, l11 = 0, l20 = 0, l21 = 0, l22 = 0;
        bool ok = true;
        double piv = m_N[0];
        ok = piv > LP_LMC_PIVOT_EPS * m_N[0];
        if (ok) {
            l00 = sqrt(piv); l10 = m_N[3] / l00; l20 = m_N[6] / l00;
            piv = m_N[4] - l10 * l10;
            ok = piv > LP_LMC_PIVOT_EPS * m_N[4];
        }
        if (ok) {
            l11 = sqrt(piv); l21 = (m_N[7] - l20 * l10) / l11;
            piv = m_N[8] - (l20 * l20 + l21 * l21);
            ok = piv > LP_LMC_PIVOT_EPS * m_N[8];
        }
        m_st[0] = ok ? 0.0 : 1.0;
        if (ok) {
            l22 = sqrt(piv);
            // L^-1 (lower) and N^-1 = L^-T L^-1
            const double i00 = 1 / l00, i11 = 1 / l11, i22 = 1 / l22;
            const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
            m33 Ni;
            Ni.m[0] = i00 * i00 + i10 * i10 + i20 * i20; Ni.m[1] = i10 * i11 + i20 * i21; Ni.m[2] = i20 * i22;
            Ni.m[4] = i11 * i11 + i21 * i21; Ni.m[5] = i21 * i22; Ni.m[8] = i22 * i22;
            Ni.m[3] = Ni.m[1]; Ni.m[6] = Ni.m[2]; Ni.m[7] = Ni.m[5];
            m33 Je;                                                      // [Jang / rho | -e / rho^2]
#pragma unroll
            for (int r = 0; r < 3; ++r) { Je.m[3 * r] = m_J[2 * r] / rho; Je.m[3 * r + 1] = m_J[2 * r + 1] / rho; Je.m[3 * r + 2] = -m_e[r] / (rho * rho); }
            const m33 Jth = mul33(mul33(ldm33(RIs + 9 * nPh), Ric), Je);
            const m33 Y = mul33(Jth, Ni);
            lmc_st33(m_G, Y);
            m_G[9] = Ni.m[6]; m_G[10] = Ni.m[7]; m_G[11] = Ni.m[8];
            const m33 Jw = mul33(tr33(ldm33(m_RG)), Jth);
            const m33 Ar = mul33(Y, tr33(Jth)), Aw = mul33(mul33(Jw, Ni), tr33(Jw));
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    m_noise[3 * i + j] = sig2 * (0.5 * (Ar.m[3 * i + j] + Ar.m[3 * j + i]));
                    m_noise[9 + 3 * i + j] = sig2 * (0.5 * (Aw.m[3 * i + j] + Aw.m[3 * j + i]));
                }
            m_noise[18] = sig2 * Ni.m[8];
        }
    }
    __syncthreads();
    const bool ok = m_st[0] == 0.0;

    if (ok) {
        // ---- 3  Q_i, then the seven rows of every non-zero column
        if (tid < L) {
            const double* hf = Hfs + 6 * tid;
            const double* w = Ws + 6 * tid;
            m33 B;                                                       // Hf_i^T W_i
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) B.m[3 * a + c] = hf[a] * w[c] + hf[3 + a] * w[3 + c];
            const m33 RI = ldm33(RIs + 9 * tid);
            double* q = Qs + 12 * tid;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const d3 g = mk3(m_G[3 * r] * B.m[0] + m_G[3 * r + 1] * B.m[3] + m_G[3 * r + 2] * B.m[6], m_G[3 * r] * B.m[1] + m_G[3 * r + 1] * B.m[4] + m_G[3 * r + 2] * B.m[7],
                                 m_G[3 * r] * B.m[2] + m_G[3 * r + 1] * B.m[5] + m_G[3 * r + 2] * B.m[8]);    // row r of [Y; (N^-1)_2] B
                q[3 * r] = g.x * RI.m[0] + g.y * RI.m[3] + g.z * RI.m[6];
                q[3 * r + 1] = g.x * RI.m[1] + g.y * RI.m[4] + g.z * RI.m[7];
                q[3 * r + 2] = g.x * RI.m[2] + g.y * RI.m[5] + g.z * RI.m[8];
            }
        }
        __syncthreads();
        const m33 RGt = tr33(ldm33(m_RG));
        if (tid < nPh) {
            const int j = tid;
            double S[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) S[k] = 0.0;
            for (int i = j + 1; i <= nPh; ++i)
#pragma unroll
                for (int k = 0; k < 12; ++k) S[k] += Qs[12 * i + k];
            const m33 RIk = ldm33(RIs + 9 * nPh), RIj = ldm33(RIs + 9 * (j + 1));
            // D = (RI_nPh - S[0:3]) RI_{j+1}^T (3 x 3), a = -S[3] RI_{j+1}^T (1 x 3)
            m33 D;
            d3 a;
            {
                m33 U;
#pragma unroll
                for (int k = 0; k < 9; ++k) U.m[k] = RIk.m[k] - S[k];
                D = mul33(U, tr33(RIj));
                a = scl3(-1.0, mv33(RIj, mk3(S[9], S[10], S[11])));
            }
            // E_j = [ [X_{j+1} x] | -R_j ]
            const m33 Ex = skew33(ld3(Xs + 3 * (j + 1))), Ep = scl33(-1.0, ldm33(Rs + 9 * j));
            const m33 Mx = mul33(D, Ex), Mp = mul33(D, Ep);
            const m33 Wx = mul33(RGt, Mx), Wp = mul33(RGt, Mp);
            const d3 ax = mk3(a.x * Ex.m[0] + a.y * Ex.m[3] + a.z * Ex.m[6], a.x * Ex.m[1] + a.y * Ex.m[4] + a.z * Ex.m[7], a.x * Ex.m[2] + a.y * Ex.m[5] + a.z * Ex.m[8]);
            const d3 ap = mk3(a.x * Ep.m[0] + a.y * Ep.m[3] + a.z * Ep.m[6], a.x * Ep.m[1] + a.y * Ep.m[4] + a.z * Ep.m[7], a.x * Ep.m[2] + a.y * Ep.m[5] + a.z * Ep.m[8]);
            double* r0 = rows + LP_LMC_ROWS * (6 + 6 * j);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    r0[LP_LMC_ROWS * c + r] = Mx.m[3 * r + c]; r0[LP_LMC_ROWS * c + 3 + r] = Wx.m[3 * r + c];
                    r0[LP_LMC_ROWS * (3 + c) + r] = Mp.m[3 * r + c]; r0[LP_LMC_ROWS * (3 + c) + 3 + r] = Wp.m[3 * r + c];
                }
            }
            r0[6] = ax.x; r0[LP_LMC_ROWS + 6] = ax.y; r0[2 * LP_LMC_ROWS + 6] = ax.z;
            r0[3 * LP_LMC_ROWS + 6] = ap.x; r0[4 * LP_LMC_ROWS + 6] = ap.y; r0[5 * LP_LMC_ROWS + 6] = ap.z;
        } else if (tid == 64) {
            const m33 Hx = scl33(-1.0, mul33(RGt, skew33(sub3(ld3(prc), ld3(xk1k + 4)))));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    rows[LP_LMC_ROWS * c + r] = 0.0; rows[LP_LMC_ROWS * c + 3 + r] = Hx.m[3 * r + c];
                    rows[LP_LMC_ROWS * (3 + c) + r] = 0.0; rows[LP_LMC_ROWS * (3 + c) + 3 + r] = -RGt.m[3 * r + c];
                }
                rows[LP_LMC_ROWS * c + 6] = 0.0; rows[LP_LMC_ROWS * (3 + c) + 6] = 0.0;
            }
        }
        __syncthreads();

        // ---- 4  T = P_nz rows^T
        if (tid < nz) {
            const double* pc = P + lmc_col(tid, cbase);
            double acc[LP_LMC_ROWS];
#pragma unroll
            for (int r = 0; r < LP_LMC_ROWS; ++r) acc[r] = 0.0;
#pragma unroll 4
            for (int k = 0; k < nz; ++k) {
                const double pv = pc[(size_t)lmc_col(k, cbase) * ld];
#pragma unroll
                for (int r = 0; r < LP_LMC_ROWS; ++r) acc[r] = fma(pv, rows[k * LP_LMC_ROWS + r], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < LP_LMC_ROWS; ++r) Ts[tid * LP_LMC_ROWS + r] = acc[r];
        }
        __syncthreads();

        // ---- 5  the shares of the thirteen groups, then their sum in a fixed order
        if (tid < LP_LMC_GROUPS * LP_LMC_ENTS) {
            const int g = tid / LP_LMC_ENTS, ent = tid - LP_LMC_ENTS * g;
            const int blk = ent / 9, in = ent - 9 * blk;
            const int i = ent == 18 ? 6 : 3 * blk + in / 3, j = ent == 18 ? 6 : 3 * blk + in % 3;
            double cij = 0.0, cji = 0.0;
            for (int e = g; e < nz; e += LP_LMC_GROUPS) {
                cij = fma(rows[e * LP_LMC_ROWS + i], Ts[e * LP_LMC_ROWS + j], cij);
                cji = fma(rows[e * LP_LMC_ROWS + j], Ts[e * LP_LMC_ROWS + i], cji);
            }
            part[2 * tid] = cij; part[2 * tid + 1] = cji;
        }
        __syncthreads();
    }
    if (tid < LP_LMC_ENTS) {
        double v = qnan;
        if (ok) {
            double cij = part[2 * tid], cji = part[2 * tid + 1];
#pragma unroll
            for (int g = 1; g < LP_LMC_GROUPS; ++g) { cij += part[2 * (LP_LMC_ENTS * g + tid)]; cji += part[2 * (LP_LMC_ENTS * g + tid) + 1]; }
            v = 0.5 * (cij + cji) + m_noise[tid];
            if (tid == 18) v = sqrt(v);
        }
        rec[tid == 18 ? 3 : 10 + tid] = (unsigned long long)__double_as_longlong(v);
    } else if (tid == 64) {
        const d3 pr = ld3(prc);
        const d3 pw = mv33(tr33(ldm33(m_RG)), sub3(pr, ld3(xk1k + 4)));
        rec[0] = (unsigned long long)(unsigned)f | ((unsigned long long)(unsigned)L << 32);
        rec[1] = ok ? 0ull : 1ull;
        rec[2] = (unsigned long long)__double_as_longlong(rho);
        rec[4] = (unsigned long long)__double_as_longlong(pr.x); rec[5] = (unsigned long long)__double_as_longlong(pr.y);
        rec[6] = (unsigned long long)__double_as_longlong(pr.z);
        rec[7] = (unsigned long long)__double_as_longlong(pw.x); rec[8] = (unsigned long long)__double_as_longlong(pw.y);
        rec[9] = (unsigned long long)__double_as_longlong(pw.z);
    }
    __syncthreads();

    // ---- 6  the record
    if (tid < LP_LMC_WORDS) o[tid] = rec[tid];
}
