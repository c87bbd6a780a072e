// landmarks.hip — Updater::update's landmark cloud (Updater.cc:78-87,430-448,458): the points the reference publishes on /rvio/landmarks.
//
// Launched behind the update (update_global_dev) when the cloud is enabled (rvio_hip_set_landmarks).  Everything it reads is in HBM already:
// the per-feature kernel's accept flags and refined (phi, psi, rho), the hand-over table the update consumed, the clone states of xk1k (the
// buffer the update read: untouched until augcomp_kernel2 rewrites it) and qG, pG of xk1k1.  One workgroup per instance (gridDim.z = B), one
// lane per feature slot, chunks of blockDim.x slots.
//
// A feature is in the cloud when it passed the chi^2 gate AND rho > 0 (Updater.cc:422,430), in hand-over order.  Its point is
//   pfk = R_k (R_ic (1/rho) e + t_ic) + t_k,   e = (cos phi sin psi, sin phi, cos phi cos psi),
// (R_k, t_k) = mRelPosesToFirst.tail(7): the end of the feature's relative-pose chain (Updater.cc:114-131), carried as normalised quaternions
// in the reference's operation order (feat_build_body's U1 carries rotation matrices instead: the same rotations up to rounding, and the
// cloud is compared against the reference's own points).  p_world = R(qG)^T (pfk - pG) is System.cc:341's map of pk to pGk.
//
// Compaction without atomics: a 64-bit ballot of the membership flag, the lane's rank inside its wave, the per-wave counts through LDS.
#define LM_MAX_T 1024

struct LmOut { int* count; int* feat; double* p_r; double* p_w; size_t bs; };   // one instance's cloud; instance z lies z * bs bytes behind

__global__ __launch_bounds__(LM_MAX_T) void landmark_kernel(DevCfg cfg, int n, const double* __restrict__ xk1k, const double* __restrict__ xk1k1,
                                                           const int* n_feat_ptr, const unsigned char* types, const int* lens,
                                                           const int* acc, const double* pfinv, size_t bs, BatchIn bin, LmOut out, const CamCal* __restrict__ cal) {
    __shared__ int wave_cnt[LM_MAX_T / 64];
    const int z = blockIdx.z;
    xk1k = zoffi(xk1k, bs, z); xk1k1 = zoffi(xk1k1, bs, z); acc = zoffi(acc, bs, z); pfinv = zoffi(pfinv, bs, z);
    n_feat_ptr = zoffi(n_feat_ptr, bin.n_feat, z); types = zoffi(types, bin.types, z); lens = zoffi(lens, bin.len, z);
    int* count = zoffi(out.count, out.bs, z);
    int* feat = zoffi(out.feat, out.bs, z);
    double* p_r = zoffi(out.p_r, out.bs, z);
    double* p_w = zoffi(out.p_w, out.bs, z);
    const int nf = min(max(*n_feat_ptr, 0), cfg.Fu);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const CamCal cam = cam_of(cfg, cal, z);
    const m33 Ric = ldm33(cam.Ric);
    const d3 tic = ld3(cam.tic);
    const m33 RG = q2r(ldq(xk1k1));
    const d3 pG = ld3(xk1k1 + 4);
    int base = 0;   // members in the chunks before this one
    for (int f0 = 0; f0 < nf; f0 += blockDim.x) {
        const int f = f0 + threadIdx.x;
        bool mem = false;
        d3 pr = mk3(0, 0, 0), pw = mk3(0, 0, 0);
        if (f < nf && acc[f] > 0) {
            const unsigned char type = types[f];
            const int nPh = lens[f] - 1;
            const double phi = pfinv[3 * f], psi = pfinv[3 * f + 1], rho = pfinv[3 * f + 2];
            // (an accepted feature always has a chain the window holds: feat_build_body rejects the others — checked again, the reads stay in the state)
            if (rho > 0 && nPh >= 1 && nPh <= n && (type == '1' || type == '2')) {
                mem = true;
                const double* rel = xk1k + 26 + (type == '1' ? 7 * (n - nPh) : 0);   // xk1k.tail(7 nPh) / xk1k.block(26, 0, 7 nPh, 1)
                q4 qI = ldq(rel);
                d3 tI = scl3(-1.0, mv33(q2r(qI), ld3(rel + 4)));
                for (int i = 1; i < nPh; ++i) {   // Updater.cc:126-131
                    const q4 qi = ldq(rel + 7 * i);
                    const m33 Ri = q2r(qi);
                    tI = mv33(Ri, sub3(tI, ld3(rel + 7 * i + 4)));
                    qI = qmul(qi, qI);
                }
                const d3 e = mk3(cos(phi) * sin(psi), sin(phi), cos(phi) * cos(psi));   // Updater.cc:165
                const d3 pf1 = add3(mv33(Ric, scl3(1 / rho, e)), tic);                  // Updater.cc:440-441
                pr = add3(mv33(q2r(qI), pf1), tI);                                     // Updater.cc:442
                pw = mv33(tr33(RG), sub3(pr, pG));                                     // System.cc:341
            }
        }
        const unsigned long long bal = __ballot(mem);
        if (lane == 0) wave_cnt[w] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
        for (int i = 0; i < nw; ++i) { const int c = wave_cnt[i]; if (i < w) off += c; tot += c; }
        if (mem) {
            const int o = off + __popcll(bal & ((1ull << lane) - 1ull));
            feat[o] = f;
            st3(p_r + 3 * o, pr);
            st3(p_w + 3 * o, pw);
        }
        base += tot;
        __syncthreads();   // (wave_cnt is rewritten by the next chunk)
    }
    if (threadIdx.x == 0) *count = base;
}
