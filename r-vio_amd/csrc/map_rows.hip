// map_rows.hip — map landmarks (rvio_hip_update_map[_dev] of include/rvio_hip.h): pixel observations of KNOWN world points — a surveyed marker
// corner, a fiducial's corners, a 2D-3D match against a prior map — made in an image the filter consumed `age` frames ago, linearised against
// the camera pose the state still holds for that image and handed to aux_update_kernel (aux_update.hip, unchanged) as a RESIDUAL-mode
// measurement of two rows per point, like fix_past.hip does for a delayed pose fix.  The raw measurement is the pixel: every point keeps its own
// information and its own chi-square gate, which is formed here against P as the call finds it — the first kernel of the family that reads P.
//
// Frames and chain are those of fix_past.hip: clone i holds (q_i, p_i), C_i = R(q_i), the age a = 0 .. n counts images back from {R},
//   A_0 = I, t_0 = 0;   A_m = A_{m-1} C_{n-m},   t_m = t_{m-1} - A_m p_{n-m}      (m = 1 .. a)
// With R_G = R(qG), f = p_w and the instance's calibration (Rci, tci):
//   w   = R_G f + pG                     the point in {R}
//   p_I = A_a^T (w - t_a)                in the IMU frame at the image a back
//   p_C = Rci p_I + tci,  depth = p_C.z
//   h   = (p_C.x, p_C.y) / depth         normalised image coordinates;   r = uv_n - h
//   J = (1 / depth) [1 0 -h.x; 0 1 -h.y],  M = J Rci A_a^T (2 x 3)
//   cols 0-2: M [(R_G f) x]   3-5: M   clone n - m (m = 1 .. a):  rotation -M [(w - t_{m-1}) x] A_{m-1}   position M A_m
// Every column not listed — 6 .. 23 and every clone older than n - a — is 0.0.  PIXELS: uv_n = undistort_pt of the pixel cast to float (what a
// tracked feature gets), the rows' sigmas are sigma / |fx| and sigma / |fy|.
//
// One launch, gridDim.z = instances, ONE workgroup of LP_MAP_WAVES = 4 waves per instance, FP64, plain C++, static LDS only.
//   1  every wave forms the chain by the in-wave scan of fix_past_kernel (lane m - 1 <-> clone n - m); wave 0 drops it into LDS
//   2  thread j < 8 <-> slot j: projection, residual, sigmas, M and the 2 x 6 head block; rejected (status 2) when the depth is below
//      LP_MAP_MIN_DEPTH or anything of it is not finite (a sigma that is not > 0 included); empty (3) at or beyond the instance's count
//   3  the rows of the candidates, TRANSPOSED in LDS (Hs[column][row]): one thread per (slot, head column) and per (slot, clone); zeros elsewhere
//   4  per-point gate: the columns that are not zero are 0 .. 5 and 24 + 6 (n - a) .. 24 + 6 n - 1, nz = 6 + 6 a <= 198 of them.  P is symmetric
//      and column-major, so y = H P is read with lane <-> column e of the compacted set (wave g: e = 64 g + lane — consecutive doubles of one
//      column of P per load) and a loop over the other index; all 16 rows ride on one pass over P.  The three entries of each slot's 2 x 2 are
//      summed over the wave (wave_sum) and then over the four waves in the order 0, 1, 2, 3: the same bits every run
//   5  thread j: S_j = H~_j P H~_j^T + I_2 from the three sums and the sigmas, its L D L^T, gamma_j = r~^T S_j^-1 r~; gated out (status 1) on a
//      non-positive pivot or, with gate_each, unless |gamma_j| < chi2inv(0.95, 2) — the feature gate's table and comparison
//   6  the 2 n_max x d rows from LDS (0.0 in the rows of every slot that is not used), r, sigma (0 / 1 there), the records, the cleared pair, the flag
// Every element of the rows is written once, by one thread.  No atomics.
//
// The kernel owns an active flag per instance: the caller's flag AND age inside 0 .. n AND at least one used slot.  aux_update_kernel gets THAT
// flag.  An instance outside the window: m = 0, applied = 0, n_used = 0, img_count = -1, every slot 3.  An instance the caller flagged inactive
// gets flag 0 and nothing else.
//
// pass: 0 is all of the above.  A later pass of the iterated update (include/rvio_hip.h, rvio_hip_set_meas_iterations) relinearises at the state
// the pass before left and keeps what pass 0 decided: a slot that was not used then keeps its status and its record untouched; a used slot
// keeps pass 0's gamma and is not gated again — steps 4 and 5's product with P are skipped — but may still become rejected by its depth at the
// new state; `active` then holds the chain's running flags.
#define MAP_USED 0
#define MAP_GATED 1
#define MAP_REJECTED 2
#define MAP_EMPTY 3

// slot record in LDS (LP_MAP_SLOT doubles): head 2 x 6 (12) | M 2 x 3 (6) | w (3) | r (2) | sigma (2) | depth | gamma
#define MAP_S_HEAD 0
#define MAP_S_M 12
#define MAP_S_W 18
#define MAP_S_R 21
#define MAP_S_SG 23
#define MAP_S_DEPTH 25
#define MAP_S_GAMMA 26

__device__ __forceinline__ d3 map_cross(d3 a, d3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ int map_col(int e, int c0) { return e < 6 ? e : c0 + e - 6; }   // column of entry e of the compacted non-zero set

// cfg / cal: the calibration source of cam_of; x / P: instance 0's, instance z lies bs bytes behind; ld: leading dimension of P; obs: instance
// 0's records, obs_bs BYTES between instances (0: shared); count: NULL (n_max each) or one per instance; age: one per instance; active: NULL or
// one flag per instance; ref_count: the frame count of {R}; H: instance 0's rows, H_bs bytes between instances; r / sigma: LP_MAP_ROWS per
// instance; rec / pair / flag: one per instance; pts: LP_MAP_POINTS per instance; n: clones now (<= LP_FIXP_NMAX)
__global__ __launch_bounds__(LP_MAP_T) void map_rows_kernel(DevCfg cfg, const CamCal* __restrict__ cal, int n, int ld, int units, int gate_each, int n_max,
                                                           const double* x, const double* P, size_t bs, const rvio_map_obs* obs, size_t obs_bs, const int* count,
                                                           const int* age, const int* active, int ref_count, double* H, size_t H_bs, double* r, double* sigma,
                                                           rvio_map_diag* rec, rvio_map_point* pts, double* pair, int* flag, int pass) {
    static_assert(LP_MAP_T == 256 && LP_FIXP_NMAX < 64 && LP_MAP_SLOT >= 27, "four waves per instance, one lane per clone");
    __shared__ double chain[LP_FIXP_CHAIN];
    __shared__ __align__(16) double Hs[LP_MAP_HS];
    __shared__ double slot[LP_MAP_POINTS * LP_MAP_SLOT];
    __shared__ double part[LP_MAP_PART];
    __shared__ int st[LP_MAP_POINTS];
    const int z = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (active && active[z] == 0) { if (tid == 0) flag[z] = 0; return; }
    const int a = age[z];
    n_max = min(max(n_max, 1), LP_MAP_POINTS);
    const int cnt = count ? min(max(count[z], 0), n_max) : n_max;
    rvio_map_point* pz = pts + LP_MAP_POINTS * (size_t)z;
    if (!(n <= LP_FIXP_NMAX && a >= 0 && a <= n)) {
        if (tid < LP_MAP_POINTS) { rvio_map_point e; e.r[0] = 0.0; e.r[1] = 0.0; e.gamma = 0.0; e.depth = 0.0; e.status = MAP_EMPTY; e.reserved = 0; pz[tid] = e; }
        if (tid == 0) {
            rvio_map_diag* out = rec + z;
            out->gamma = 0.0; out->applied = 0; out->m = 0; out->n_used = 0; out->n_obs = cnt; out->img_count = -1; out->reserved = 0;
            pair[2 * (size_t)z] = 0.0; ((long long*)pair)[2 * (size_t)z + 1] = 0;
            flag[z] = 0;
        }
        return;
    }
    x = zoffi(x, bs, z);
    P = zoffi(P, bs, z);
    obs = zoffi(obs, obs_bs, z);
    H = zoffi(H, H_bs, z);
    const int d = 24 + 6 * n;

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
        for (int off = 1; off < a; off <<= 1) {          // (uniform: a is the instance's)
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

    // ---- 2  thread j <-> slot j: projection, residual, sigmas, M, the head block
    if (tid < LP_MAP_POINTS) {
        double* s = slot + tid * LP_MAP_SLOT;
#pragma unroll
        for (int k = 0; k < LP_MAP_SLOT; ++k) s[k] = 0.0;
        int status = MAP_EMPTY;
        const int held = pass > 0 ? pz[tid].status : MAP_USED;   // what pass 0 made of the slot
        if (tid < cnt && held != MAP_USED) status = held;
        else if (tid < cnt) {
            const CamCal cam = cam_of(cfg, cal, z);
            const rvio_map_obs* o = obs + tid;
            m33 Rci;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rci.m[k] = cam.Rci[k];
            const d3 RGf = mv33(q2r(ldq(x)), ld3(o->p_w));
            const d3 w = add3(RGf, ld3(x + 4));
            const fixp_rt Ea = fixp_ld(chain, a);
            const m33 At = tr33(Ea.A);
            const d3 pC = add3(mv33(Rci, mv33(At, sub3(w, Ea.t))), mk3(cam.tci[0], cam.tci[1], cam.tci[2]));
            const double depth = pC.z, hx = pC.x / depth, hy = pC.y / depth;
            double ux = o->uv[0], uy = o->uv[1], s0 = o->sigma, s1 = o->sigma;
            if (units == RVIO_MAP_PIXELS) {
                float ox, oy;
                undistort_pt(cam, (float)ux, (float)uy, &ox, &oy);
                ux = (double)ox; uy = (double)oy;
                s0 = o->sigma / fabs((double)cam.fx); s1 = o->sigma / fabs((double)cam.fy);
            }
            const double r0 = ux - hx, r1 = uy - hy;
            const bool fin = isfinite(depth) && isfinite(hx) && isfinite(hy) && isfinite(r0) && isfinite(r1) && isfinite(s0) && isfinite(s1) && s0 > 0.0 && s1 > 0.0;
            status = (fin && depth >= LP_MAP_MIN_DEPTH) ? MAP_USED : MAP_REJECTED;
            s[MAP_S_DEPTH] = depth;
            if (status == MAP_USED) {
                const m33 RA = mul33(Rci, At);
                const double id = 1.0 / depth;
                const d3 m0 = mk3((RA.m[0] - hx * RA.m[6]) * id, (RA.m[1] - hx * RA.m[7]) * id, (RA.m[2] - hx * RA.m[8]) * id);
                const d3 m1 = mk3((RA.m[3] - hy * RA.m[6]) * id, (RA.m[4] - hy * RA.m[7]) * id, (RA.m[5] - hy * RA.m[8]) * id);
                const d3 g0 = map_cross(m0, RGf), g1 = map_cross(m1, RGf);      // m^T [v x] = (m x v)^T
                s[MAP_S_HEAD + 0] = g0.x; s[MAP_S_HEAD + 1] = g0.y; s[MAP_S_HEAD + 2] = g0.z; s[MAP_S_HEAD + 3] = m0.x; s[MAP_S_HEAD + 4] = m0.y; s[MAP_S_HEAD + 5] = m0.z;
                s[MAP_S_HEAD + 6] = g1.x; s[MAP_S_HEAD + 7] = g1.y; s[MAP_S_HEAD + 8] = g1.z; s[MAP_S_HEAD + 9] = m1.x; s[MAP_S_HEAD + 10] = m1.y; s[MAP_S_HEAD + 11] = m1.z;
                s[MAP_S_M + 0] = m0.x; s[MAP_S_M + 1] = m0.y; s[MAP_S_M + 2] = m0.z; s[MAP_S_M + 3] = m1.x; s[MAP_S_M + 4] = m1.y; s[MAP_S_M + 5] = m1.z;
                s[MAP_S_W + 0] = w.x; s[MAP_S_W + 1] = w.y; s[MAP_S_W + 2] = w.z;
                s[MAP_S_R + 0] = r0; s[MAP_S_R + 1] = r1;
                s[MAP_S_SG + 0] = s0; s[MAP_S_SG + 1] = s1;
            }
        }
        st[tid] = status;
    }
    __syncthreads();

    // ---- 3  the candidates' rows, transposed: Hs[column * LP_MAP_ROWS + row]
    {
        const int per = 24 + n;
        for (int it = tid; it < LP_MAP_POINTS * per; it += LP_MAP_T) {
            const int j = it / per, q = it - j * per;
            const double* s = slot + j * LP_MAP_SLOT;
            const bool live = st[j] == MAP_USED;
            if (q < 24) {
                double v0 = 0.0, v1 = 0.0;
                if (live && q < 6) { v0 = s[MAP_S_HEAD + q]; v1 = s[MAP_S_HEAD + 6 + q]; }
                Hs[q * LP_MAP_ROWS + 2 * j] = v0; Hs[q * LP_MAP_ROWS + 2 * j + 1] = v1;
            } else {
                const int mm = q - 23;                       // clone n - mm
                d3 r0 = mk3(0.0, 0.0, 0.0), p0 = r0, r1 = r0, p1 = r0;
                if (live && mm <= a) {
                    const fixp_rt E0 = fixp_ld(chain, mm - 1), E1 = fixp_ld(chain, mm);
                    const d3 m0 = ld3(s + MAP_S_M), m1 = ld3(s + MAP_S_M + 3);
                    const d3 v = sub3(ld3(s + MAP_S_W), E0.t);
                    const m33 A0t = tr33(E0.A), A1t = tr33(E1.A);
                    r0 = scl3(-1.0, mv33(A0t, map_cross(m0, v))); r1 = scl3(-1.0, mv33(A0t, map_cross(m1, v)));   // -(m^T [v x] A_{m-1})
                    p0 = mv33(A1t, m0); p1 = mv33(A1t, m1);                                                    // m^T A_m
                }
                double* c = Hs + (size_t)(24 + 6 * (n - mm)) * LP_MAP_ROWS + 2 * j;
                c[0] = r0.x; c[LP_MAP_ROWS] = r0.y; c[2 * LP_MAP_ROWS] = r0.z; c[3 * LP_MAP_ROWS] = p0.x; c[4 * LP_MAP_ROWS] = p0.y; c[5 * LP_MAP_ROWS] = p0.z;
                c[1] = r1.x; c[LP_MAP_ROWS + 1] = r1.y; c[2 * LP_MAP_ROWS + 1] = r1.z; c[3 * LP_MAP_ROWS + 1] = p1.x; c[4 * LP_MAP_ROWS + 1] = p1.y; c[5 * LP_MAP_ROWS + 1] = p1.z;
            }
        }
    }
    __syncthreads();

    // ---- 4  y = H P over the compacted columns, the three sums of every slot's 2 x 2
    if (pass == 0) {   // (uniform)
        const int nz = 6 + 6 * a, c0 = 24 + 6 * (n - a);
        const int e = 64 * wv + lane;
        const bool on = e < nz;
        const int ce = on ? map_col(e, c0) : 0;
        double acc[LP_MAP_ROWS];
#pragma unroll
        for (int k = 0; k < LP_MAP_ROWS; ++k) acc[k] = 0.0;
        if (64 * wv < nz) {                                  // (uniform over the wave)
            const double* pc = P + ce;
#pragma unroll 4
            for (int k = 0; k < nz; ++k) {
                const int ck = map_col(k, c0);
                const double pv = pc[(size_t)ck * ld];
#pragma unroll
                for (int q = 0; q < LP_MAP_ROWS; ++q) acc[q] = fma(pv, Hs[ck * LP_MAP_ROWS + q], acc[q]);
            }
        }
#pragma unroll
        for (int j = 0; j < LP_MAP_POINTS; ++j) {
            const double h0 = on ? Hs[ce * LP_MAP_ROWS + 2 * j] : 0.0, h1 = on ? Hs[ce * LP_MAP_ROWS + 2 * j + 1] : 0.0;
            const double q00 = wave_sum(on ? acc[2 * j] * h0 : 0.0), q01 = wave_sum(on ? acc[2 * j] * h1 : 0.0), q11 = wave_sum(on ? acc[2 * j + 1] * h1 : 0.0);
            if (lane == 0) { double* p = part + (wv * LP_MAP_POINTS + j) * 3; p[0] = q00; p[1] = q01; p[2] = q11; }
        }
    }
    __syncthreads();

    // ---- 5  thread j: the 2 x 2, its L D L^T, gamma_j, the decision, the slot's record
    if (pass > 0) {   // the statuses stand; a slot still used reports its new residual and depth beside pass 0's gamma
        if (tid < LP_MAP_POINTS && pz[tid].status == MAP_USED) {
            const double* s = slot + tid * LP_MAP_SLOT;
            const bool used = st[tid] == MAP_USED;
            rvio_map_point e;
            e.r[0] = used ? s[MAP_S_R] : 0.0; e.r[1] = used ? s[MAP_S_R + 1] : 0.0;
            e.gamma = used ? pz[tid].gamma : 0.0; e.depth = s[MAP_S_DEPTH]; e.status = st[tid]; e.reserved = 0;
            pz[tid] = e;
        }
    } else if (tid < LP_MAP_POINTS) {
        double* s = slot + tid * LP_MAP_SLOT;
        int status = st[tid];
        double gam = 0.0;
        if (status == MAP_USED) {
            double q00 = part[tid * 3], q01 = part[tid * 3 + 1], q11 = part[tid * 3 + 2];
#pragma unroll
            for (int g = 1; g < LP_MAP_WAVES; ++g) {
                const double* p = part + (g * LP_MAP_POINTS + tid) * 3;
                q00 += p[0]; q01 += p[1]; q11 += p[2];
            }
            const double s0 = s[MAP_S_SG], s1 = s[MAP_S_SG + 1];
            const double S00 = q00 / (s0 * s0) + 1.0, S01 = q01 / (s0 * s1), S11 = q11 / (s1 * s1) + 1.0;
            const double w0 = s[MAP_S_R] / s0, w1 = s[MAP_S_R + 1] / s1;
            const double d0 = S00, l = S01 / (d0 > 0 ? d0 : 1e-300), d1 = S11 - l * S01;
            const bool neg = !(d0 > 0) || !(d1 > 0);
            const double e1 = w1 - l * w0;
            gam = fabs(w0 * w0 / (d0 > 0 ? d0 : 1e-300) + e1 * e1 / (d1 > 0 ? d1 : 1e-300));
            if (neg) { status = MAP_GATED; gam = 0.0; }
            else if (gate_each && !(gam < kChi2Dev[1])) status = MAP_GATED;
            st[tid] = status;
            s[MAP_S_GAMMA] = gam;
        }
        rvio_map_point e;
        const bool seen = status == MAP_USED || status == MAP_GATED;
        e.r[0] = seen ? s[MAP_S_R] : 0.0; e.r[1] = seen ? s[MAP_S_R + 1] : 0.0;
        e.gamma = gam; e.depth = s[MAP_S_DEPTH]; e.status = status; e.reserved = 0;
        pz[tid] = e;
    }
    __syncthreads();

    // ---- 6  rows, r, sigma, the record, the flag
    const int m2 = 2 * n_max;
    for (int e = tid; e < m2 * d; e += LP_MAP_T) {
        const int row = e / d, col = e - row * d;
        H[e] = st[row >> 1] == MAP_USED ? Hs[col * LP_MAP_ROWS + row] : 0.0;
    }
    if (tid < m2) {
        const bool used = st[tid >> 1] == MAP_USED;
        const double* s = slot + (tid >> 1) * LP_MAP_SLOT;
        r[LP_MAP_ROWS * (size_t)z + tid] = used ? s[MAP_S_R + (tid & 1)] : 0.0;
        sigma[LP_MAP_ROWS * (size_t)z + tid] = used ? s[MAP_S_SG + (tid & 1)] : 1.0;
    }
    if (tid == 0) {
        int n_used = 0;
#pragma unroll
        for (int j = 0; j < LP_MAP_POINTS; ++j) n_used += st[j] == MAP_USED ? 1 : 0;
        rvio_map_diag* out = rec + z;
        out->gamma = 0.0; out->applied = 0; out->m = n_used ? m2 : 0; out->n_used = n_used; out->n_obs = cnt; out->img_count = ref_count - a; out->reserved = 0;
        pair[2 * (size_t)z] = 0.0; ((long long*)pair)[2 * (size_t)z + 1] = 0;
        flag[z] = n_used ? 1 : 0;
    }
}
