// aux_update.hip — the auxiliary EKF measurement update (rvio_hip_update_aux[_dev] of include/rvio_hip.h): at most RVIO_AUX_MAX_ROWS rows of a
// caller-linearised measurement with a FULL-WIDTH Jacobian H (m x d over the error state, d = 24 + 6 n) fused into (x, P) IN PLACE.  The
// arithmetic of Updater.cc:540-619 on whitened rows H~ = H / sigma, v~ = v / sigma (R = I):
//   T = P H~^T (d x m)    S = H~ T + I    K = T S^-1    dx = K v~    gamma = v~^T S^-1 v~
//   P+ = (I - K H~) P (I - K H~)^T + K K^T = P - K T^T - T K^T + K S K^T              (the Joseph form, multiplied out)
//      = P - K T^T + D K^T,   D = K S - T                                             (the two middle terms folded: T K^T and K S K^T share K^T)
// which holds for ANY K — an inexact S^-1 leaves P+ the covariance of the gain actually applied, the property the Joseph form is used for — and
// needs, per output element, the input element at the same place plus two rows of the d x m operands T, K, D held in LDS.  So nothing is
// double-buffered: every element of the upper triangle is read once, updated and stored together with its mirror image (P+ is symmetric
// bit for bit), and a gated-out, inactive or indefinite instance stores nothing at all.
//
// One launch per call, gridDim.z = instances, ONE workgroup of LP_AUX_T threads (eight waves) per instance: the in-place update needs every
// read of P by the T product finished before the first store, which inside one workgroup is a barrier.  MB = 4 | 16: the row count the
// register arrays are unrolled for (m <= 4: zero-velocity and velocity updates; else 16); rows m .. MB - 1 are exact zeros in H~, T, K, D.
//   1  stage H~ TRANSPOSED ([column][row], stride MB: the T product reads one column's MB entries as broadcasts) and, in VALUE mode, xi(x)
//   2  v~ = v / sigma (RESIDUAL) or z / sigma - H~ xi (VALUE), a wave per row
//   3  T: lane <-> row of P (P is column-major: a wave reads 64 consecutive doubles of a column), G = ceil(d / 64) row groups x S column
//      ranges dealt over the waves (aux_splits: G S <= 8), the S partial sums added in a fixed order
//   4  S = H~ T + I: thread <-> (entry, column range), the ranges summed in a fixed order by wave 0, which then runs the square-root-free
//      L D L^T of the feature gate (filter_kernels.hip ldlt_gamma_wave: lane <-> row in registers, v~ as one more row) and keeps L and 1 / d
//   5  gate: |gamma| < CHI_THRESHOLD[m - 1] (the feature gate's table and comparison); a non-positive pivot sets sticky error bit 8
//   6  thread <-> row i: K_i by forward / backward substitution with L (broadcast reads), D_i = K_i S - T_i, dx_i = K_i v~
//   7  state injection (Updater.cc:546-613, the lines of solve6.hip) and the pose line (augcomp_kernel2's / imu_pose_kernel's map) — in place
//   8  P+: lane <-> row i with K_i, D_i in registers, a wave per column j >= the row group's first row, four columns in flight
// Nothing beyond d rows / columns of P, m rows of H, v, sigma and 26 + 7 n states is read.
// The same body, under a template flag, is one pass of the iterated update (aux_iter_kernel, below): the device-linearised families
// relinearised against the prior, P written by the final pass alone.
// Register arrays are indexed by compile-time constants only (the rule at the head of filter_kernels2.hip).
#define AUX_NW (LP_AUX_T / 64)

__device__ __forceinline__ double aux_xi(const double* x, int c) {   // xi(x): the additive coordinates in error-state order, 0 in the rotation slots
    if (c < 24) return (c >= 3 && c < 9) ? x[c + 1] : (c >= 12 ? x[c + 2] : 0.0);
    const int p = (c - 24) / 6, o = (c - 24) % 6;
    return o >= 3 ? x[26 + 7 * p + 4 + (o - 3)] : 0.0;
}

// What the iterated form (aux_iter_kernel) gets beside the arguments of the plain one: the per-instance block of the measurement chain — the
// snapshot x0 (the state of pass 0, then the pose line: x0_ld doubles per instance, the pose at x0_ld - 7), dx (dx_ld per instance), the record
// and the running flag — and the pass: its index, the last one's, the step below which an instance is finished
struct AuxIter { double* x0; double* dx; rvio_meas_iter* rec; int* run; size_t x0_ld, dx_ld; int pass, last; double tol; };
// the state and the pose line as pass 0 found them, back from the instance's snapshot (x, pose, x0: the instance's)
__device__ __forceinline__ void aux_iter_restore(int n, double* x, double* pose, const double* x0, size_t x0_ld, int tid) {
    for (int e = tid; e < 26 + 7 * n; e += LP_AUX_T) x[e] = x0[e];
    if (tid < 7) pose[tid] = x0[x0_ld - 7 + tid];
}

// x / P / pose / meta: instance 0's, instance z lies bs bytes behind; H / v / sg: instance 0's, H_bs / v_bs / sg_bs BYTES between instances
// (0: shared); active: NULL or one flag per instance; diag: two 8-byte words per instance (gamma, applied)
// IT: one pass of the iterated update (include/rvio_hip.h, rvio_hip_set_meas_iterations): the gain is formed against P, which no pass but the
// final one writes — so P is the prior covariance at every pass — and the residual is referred to the prior, v~ + H~ dx, with dx the correction
// the previous pass left in the block.  What differs from the plain form stands under `if constexpr (IT)`; the plain form compiles without it.
//   1  pass 0 snapshots x and the pose line into the block; dx (0 at pass 0) is staged in LDS
//   2  v~ += H~ dx, the wave-per-row reduction of VALUE mode
//   5  the chi-square gate at pass 0 only (there v~ is the innovation); a non-positive pivot at a later pass writes x and the pose back from
//      the snapshot: (x0, P0) stay
//   6+ step = max |dx_new - dx|, the maximum over the waves' maxima (exact, so the same bits in any order); final = step < tol or the last pass
//   7  the injection reads the snapshot (x0 + dx_new, never chained) and writes x; dx_new goes to the block
//   8  on the final pass only
// Flags: pass 0 runs where the caller's `active` (the rows kernel's own flag, which is the caller's AND its own test) says so and leaves run[z] = 1
// unless the instance is finished; a later pass runs where run[z] is set.  A finished instance — converged, last pass, gated out, refused — has
// run[z] = 0: the rows kernel of the next pass gets run[] as its flags, and neither kernel touches the instance again.  A rows kernel that
// refuses at a later pass an instance it accepted at pass 0 (every map point behind the camera at the new linearisation) ends it like a
// non-positive pivot: the snapshot back, applied = 0.
template <int MB, bool IT>
__device__ __forceinline__ void aux_update_body(int n, int ld, int m, int mode, int gate, double* x, double* P, double* pose, FilterMeta* meta, size_t bs,
                                                const double* H, size_t H_bs, const double* v, size_t v_bs, const double* sg, size_t sg_bs,
                                                const int* active, double* diag, const AuxIter& it) {
    extern __shared__ __align__(16) double aux_dyn[];
    constexpr int TS = MB + 1;   // row stride of T, K, D, the partial sums and the m x m matrices: odd, lane-indexed rows hit distinct banks
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    diag += 2 * (size_t)z;
    if constexpr (IT) {
        if (it.pass == 0 ? (active && active[z] == 0) : it.run[z] == 0) {
            if (it.pass == 0 && tid == 0) {
                diag[0] = 0.0; ((long long*)diag)[1] = 0;
                rvio_meas_iter e; e.step = 0.0; e.gamma0 = 0.0; e.iterations = 0; e.converged = 0;
                it.rec[z] = e; it.run[z] = 0;
            }
            return;
        }
    } else {
        if (active && active[z] == 0) {
            if (tid == 0) { diag[0] = 0.0; ((long long*)diag)[1] = 0; }
            return;
        }
    }
    x = zoffi(x, bs, z); P = zoffi(P, bs, z); pose = zoffi(pose, bs, z); meta = zoffi(meta, bs, z);
    H = zoffi(H, H_bs, z); v = zoffi(v, v_bs, z); sg = zoffi(sg, sg_bs, z);
    const int d = 24 + 6 * n, G = (d + 63) >> 6, S = aux_splits(G);
    // LDS (launch_plan.h aux_lds_doubles): Hs | Tl | U | Sm | Lm | dinv | vt | xi | dxs | misc;  U: the partial sums of T, then those of S, then K | D
    double* Hs = aux_dyn;
    double* Tl = Hs + (size_t)d * MB;
    double* U = Tl + (size_t)d * TS;
    double* Sm = U + aux_u_doubles(d, MB);
    double* Lm = Sm + MB * TS;
    double* dinv = Lm + MB * TS;
    double* vt = dinv + MB;
    double* xi = vt + MB;
    double* dxs = xi + d;
    double* misc = dxs + d;
    double* Kl = U;
    double* Dl = U + (size_t)d * TS;
    double* dxp = misc + 8;      // (IT: launch_plan.h aux_iter_lds_doubles) the correction of the previous pass
    double* x0 = nullptr;
    double* dxg = nullptr;
    if constexpr (IT) {
        x0 = it.x0 + it.x0_ld * (size_t)z; dxg = it.dx + it.dx_ld * (size_t)z;
        if (it.pass > 0 && active && active[z] == 0) {   // the rows kernel refused at this linearisation what it accepted at pass 0
            aux_iter_restore(n, x, pose, x0, it.x0_ld, tid);
            if (tid == 0) { diag[0] = it.rec[z].gamma0; ((long long*)diag)[1] = 0; it.rec[z].converged = 0; it.run[z] = 0; }
            return;
        }
    }
    // ---- 1
    for (int e = tid; e < m * d; e += LP_AUX_T) { const int r = e / d, c = e - r * d; Hs[c * MB + r] = H[e] / sg[r]; }
    for (int e = tid; e < (MB - m) * d; e += LP_AUX_T) { const int r = e / d, c = e - r * d; Hs[c * MB + m + r] = 0.0; }
    if (mode) for (int c = tid; c < d; c += LP_AUX_T) xi[c] = aux_xi(x, c);
    if constexpr (IT) {
        if (it.pass == 0) {
            for (int e = tid; e < 26 + 7 * n; e += LP_AUX_T) x0[e] = x[e];
            if (tid < 7) x0[it.x0_ld - 7 + tid] = pose[tid];
        }
        for (int c = tid; c < d; c += LP_AUX_T) dxp[c] = it.pass == 0 ? 0.0 : dxg[c];
    }
    __syncthreads();
    // ---- 2
    for (int r = wv; r < MB; r += AUX_NW) {
        double s = 0.0;
        if (mode && r < m) {
            for (int c = lane; c < d; c += 64) s += Hs[c * MB + r] * xi[c];
            s = wave_sum(s);
        }
        if constexpr (IT) {
            double t = 0.0;
            if (it.pass > 0 && r < m) {   // (uniform over the wave)
                for (int c = lane; c < d; c += 64) t += Hs[c * MB + r] * dxp[c];
                t = wave_sum(t);
            }
            if (lane == 0) vt[r] = (r < m) ? (v[r] / sg[r] - s) + t : 0.0;
        } else {
            if (lane == 0) vt[r] = (r < m) ? v[r] / sg[r] - s : 0.0;
        }
    }
    // ---- 3
    if (wv < G * S) {
        const int g = wv / S, s = wv - g * S, i = 64 * g + lane, ic = min(i, d - 1);
        const int chunk = (d + S - 1) / S, c0 = s * chunk, c1 = min(d, c0 + chunk);
        double acc[MB];
#pragma unroll
        for (int r = 0; r < MB; ++r) acc[r] = 0.0;
        const double* pc = P + ic;
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            const double pv = pc[(size_t)c * ld];
#pragma unroll
            for (int r = 0; r < MB; ++r) acc[r] = fma(pv, Hs[c * MB + r], acc[r]);
        }
        if (i < d) {
#pragma unroll
            for (int r = 0; r < MB; ++r) U[((size_t)s * d + i) * TS + r] = acc[r];
        }
    }
    __syncthreads();
    for (int e = tid; e < d * MB; e += LP_AUX_T) {
        const int i = e / MB, r = e - i * MB;
        double a = U[(size_t)i * TS + r];
        for (int s = 1; s < S; ++s) a += U[((size_t)s * d + i) * TS + r];
        Tl[i * TS + r] = a;
    }
    __syncthreads();
    // ---- 4
    constexpr int NQ = (LP_AUX_T / (MB * MB)) < 8 ? (LP_AUX_T / (MB * MB)) : 8;   // column ranges of the S product
    {
        const int e = tid % (MB * MB), q = tid / (MB * MB);
        if (q < NQ) {
            const int r = e / MB, s = e - r * MB;
            const int chunk = (d + NQ - 1) / NQ, c0 = q * chunk, c1 = min(d, c0 + chunk);
            double a = 0.0;
            for (int c = c0; c < c1; ++c) a = fma(Hs[c * MB + r], Tl[c * TS + s], a);
            U[q * MB * MB + e] = a;
        }
    }
    __syncthreads();
    if (wv == 0) {
        for (int e = lane; e < MB * MB; e += 64) {
            const int r = e / MB, s = e - r * MB;
            double a = U[e];
#pragma unroll
            for (int q = 1; q < NQ; ++q) a += U[q * MB * MB + e];
            Sm[r * TS + s] = a + (r == s ? 1.0 : 0.0);
        }
        // (one wave: its LDS operations complete in program order; the fence keeps the compiler from moving them across the phase boundary)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // L D L^T: lane i < m holds row i of the lower triangle of S, lane m the row v~; columns stay unscaled (row[k] = l_ik d_k)
        double row[MB];
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            const double sv = Sm[min(lane, MB - 1) * TS + j], rv = vt[j];
            row[j] = (j < m && lane <= m && (lane == m || j <= lane)) ? (lane == m ? rv : sv) : 0.0;
        }
        double gl = 0.0;
        bool neg = false;
#pragma unroll
        for (int k = 0; k < MB; ++k) {
            if (k < m) {
                const double dk = readlane_f64(row[k], k);
                neg |= !(dk > 0);
                const double rdk = 1.0 / (dk > 0 ? dk : 1e-300);
                const double lik = row[k] * rdk;        // l_ik (rows i > k); lane m: w_k / d_k
                gl += row[k] * lik;                     // lane m: w_k^2 / d_k
#pragma unroll
                for (int j = k + 1; j < MB; ++j) row[j] -= lik * readlane_f64(row[k], j);
                if (lane < m) Lm[lane * TS + k] = lik;  // (entries k >= lane are never read)
                if (lane == 0) dinv[k] = rdk;
            }
        }
        const double gam = fabs(readlane_f64(gl, m));
        // S = H~ P H~^T + I is positive definite whenever P is positive semi-definite: a non-positive pivot means the covariance handed in is not
        bool apply;
        if constexpr (IT) apply = !neg && (!gate || it.pass > 0 || gam < kChi2Dev[m - 1]);
        else apply = !neg && (!gate || gam < kChi2Dev[m - 1]);
        if (lane == 0) {
            if (neg) atomicOr(&meta->err, 8);
            misc[0] = apply ? 1.0 : 0.0;
            if constexpr (IT) {   // the pair keeps pass 0's gamma (the rows kernel of a later pass cleared it)
                if (it.pass == 0) it.rec[z].gamma0 = gam;
                diag[0] = it.pass == 0 ? gam : it.rec[z].gamma0; ((long long*)diag)[1] = apply ? 1 : 0;
            } else {
                diag[0] = gam; ((long long*)diag)[1] = apply ? 1 : 0;
            }
        }
    }
    __syncthreads();
    // ---- 5
    if constexpr (IT) {
        if (misc[0] == 0.0) {   // finished: gated out at pass 0 (nothing is written), or a non-positive pivot (a later pass: the snapshot back)
            if (it.pass > 0) aux_iter_restore(n, x, pose, x0, it.x0_ld, tid);
            if (tid == 0) {
                rvio_meas_iter* e = it.rec + z;
                if (it.pass == 0) e->step = 0.0;
                e->iterations = it.pass + 1; e->converged = 0;
                it.run[z] = 0;
            }
            return;
        }
    }
    if (misc[0] == 0.0) return;
    // ---- 6
    if (tid < d) {
        double t[MB], k[MB];
#pragma unroll
        for (int r = 0; r < MB; ++r) t[r] = Tl[tid * TS + r];
        // L y = t,  z = D^-1 y,  L^T k = z   (S k = t: row tid of K = T S^-1, S symmetric)
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            double a = t[j];
            if (j < m) {
#pragma unroll
                for (int c = 0; c < j; ++c) a -= Lm[j * TS + c] * k[c];
            }
            k[j] = (j < m) ? a : 0.0;
        }
#pragma unroll
        for (int j = 0; j < MB; ++j) if (j < m) k[j] *= dinv[j];
#pragma unroll
        for (int j = MB - 1; j >= 0; --j) {
            if (j < m) {
                double a = k[j];
#pragma unroll
                for (int c = j + 1; c < MB; ++c) if (c < m) a -= Lm[c * TS + j] * k[c];
                k[j] = a;
            }
        }
        double dxi = 0.0;
#pragma unroll
        for (int r = 0; r < MB; ++r) {
            double a = -t[r];
            if (r < m) {
#pragma unroll
                for (int c = 0; c < MB; ++c) if (c < m) a = fma(k[c], Sm[c * TS + r], a);
            }
            Kl[tid * TS + r] = k[r];
            Dl[tid * TS + r] = (r < m) ? a : 0.0;
            dxi = fma(k[r], vt[r], dxi);
        }
        dxs[tid] = dxi;
    }
    __syncthreads();
    // xs: what the injection reads.  The plain form and pass 0 (x0 = x there): the state in place; a later pass: the snapshot
    const double* xs = x;
    bool final = true;
    if constexpr (IT) {
        // step = max |dx_new - dx|: per wave by exchange, then over the waves' maxima in S's place (S and L are read no more); a difference that
        // is not a number counts as an infinite step
        double a = 0.0;
        for (int c = tid; c < d; c += LP_AUX_T) { const double e = fabs(dxs[c] - dxp[c]); a = fmax(a, e == e ? e : (double)INFINITY); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off, 64));
        if (lane == 0) Sm[wv] = a;
        __syncthreads();
        double step = Sm[0];
#pragma unroll
        for (int w = 1; w < AUX_NW; ++w) step = fmax(step, Sm[w]);
        final = step < it.tol || it.pass == it.last;   // (uniform over the workgroup)
        if (it.pass > 0) xs = x0;
        for (int c = tid; c < d; c += LP_AUX_T) dxg[c] = dxs[c];
        if (tid == 0) {
            rvio_meas_iter* e = it.rec + z;
            e->step = step; e->iterations = it.pass + 1; e->converged = step < it.tol ? 1 : 0;
            it.run[z] = final ? 0 : 1;
        }
    }
    // ---- 7   (each thread reads the slots it rewrites; thread 0 keeps what the pose line needs)
    if (tid == 0) {
        const double* dx = dxs;
        const q4 qG = qmul(small_q(dx[0], dx[1], dx[2]), ldq(xs));
        stq(x, qG);
        for (int i = 0; i < 6; ++i) x[4 + i] = dx[3 + i] + xs[4 + i];
        st3(x + 7, unit3(ld3(x + 7)));
        // (System::initialize leaves qk all zero until the first composition, and everything reads it through QuatToRot, which gives I: the
        // identity it stands for is what the error quaternion multiplies — QuatMul would normalise 0 / 0)
        q4 qk0 = ldq(xs + 10);
        if (qk0.x == 0.0 && qk0.y == 0.0 && qk0.z == 0.0 && qk0.w == 0.0) qk0.w = 1.0;
        const q4 qk = qmul(small_q(dx[9], dx[10], dx[11]), qk0);
        stq(x + 10, qk);
        for (int i = 0; i < 12; ++i) x[14 + i] = dx[12 + i] + xs[14 + i];
        const q4 qkG = qmul(qk, qG);
        const d3 pGk = mv33(tr33(q2r(qG)), sub3(ld3(x + 14), ld3(x + 4)));   // pose line (System.cc:371-374)
        st3(pose, pGk); stq(pose + 3, qkG);
    }
    for (int p = tid - 64; p >= 0 && p < n; p += LP_AUX_T - 64) {
        const double* dx = dxs;
        stq(x + 26 + 7 * p, qmul(small_q(dx[24 + 6 * p], dx[24 + 6 * p + 1], dx[24 + 6 * p + 2]), ldq(xs + 26 + 7 * p)));
        for (int i = 0; i < 3; ++i) x[26 + 7 * p + 4 + i] = dx[24 + 6 * p + 3 + i] + xs[26 + 7 * p + 4 + i];
    }
    if constexpr (IT) { if (!final) return; }
    // ---- 8   (only elements on and above the diagonal are read; the mirror stores go below it)
    for (int g = 0; g < G; ++g) {
        const int i = 64 * g + lane, ic = min(i, d - 1);
        double ki[MB], di[MB];
#pragma unroll
        for (int r = 0; r < MB; ++r) { ki[r] = Kl[ic * TS + r]; di[r] = Dl[ic * TS + r]; }
        for (int j0 = 64 * g + wv; j0 < d; j0 += 4 * AUX_NW) {
            double pj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u * AUX_NW, d - 1);
                pj[u] = P[(size_t)min(ic, j) + (size_t)j * ld];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * AUX_NW;
                if (j < d) {                                   // (uniform)
                    double a = pj[u];
#pragma unroll
                    for (int r = 0; r < MB; ++r) a = fma(-ki[r], Tl[j * TS + r], a);
#pragma unroll
                    for (int r = 0; r < MB; ++r) a = fma(di[r], Kl[j * TS + r], a);
                    pj[u] = a;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * AUX_NW;
                if (j < d && i <= j && i < d) {
                    P[(size_t)i + (size_t)j * ld] = pj[u];
                    if (i != j) P[(size_t)j + (size_t)i * ld] = pj[u];
                }
            }
        }
    }
}

template <int MB>
__global__ __launch_bounds__(LP_AUX_T) void aux_update_kernel(int n, int ld, int m, int mode, int gate, double* x, double* P, double* pose,
                                                              FilterMeta* meta, size_t bs, const double* H, size_t H_bs, const double* v,
                                                              size_t v_bs, const double* sg, size_t sg_bs, const int* active, double* diag) {
    aux_update_body<MB, false>(n, ld, m, mode, gate, x, P, pose, meta, bs, H, H_bs, v, v_bs, sg, sg_bs, active, diag, AuxIter{});
}
// one pass of the iterated update; dynamic LDS: launch_plan.h aux_iter_lds_doubles
template <int MB>
__global__ __launch_bounds__(LP_AUX_T) void aux_iter_kernel(int n, int ld, int m, int mode, int gate, double* x, double* P, double* pose,
                                                            FilterMeta* meta, size_t bs, const double* H, size_t H_bs, const double* v,
                                                            size_t v_bs, const double* sg, size_t sg_bs, const int* active, double* diag, AuxIter it) {
    aux_update_body<MB, true>(n, ld, m, mode, gate, x, P, pose, meta, bs, H, H_bs, v, v_bs, sg, sg_bs, active, diag, it);
}
