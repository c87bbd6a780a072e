// launch_plan.h — the launch geometry of a handle as a function of (max_track_len, n_features, batch): every dynamic-LDS size, the kernel
// variants and the LDS-or-global decisions that rvio_hip_create / rvio_hip_create_batch derive from a configuration.
//
// Plain C++: create_impl (rvio_hip.hip) calls launch_plan() and applies what it returns, and tests/hostemu/plan_emu.cpp compiles THIS text with
// g++ and sweeps every accepted configuration on the CPU (tests/test_launch_plan.py) — a configuration whose footprint does not fit a CU is
// found by arithmetic, not by a failed launch.  The one input that is not arithmetic is the STATIC LDS of each kernel, which the compiler
// decides: create_impl reads it from the loaded code object (hipFuncGetAttributes), the test from the notes of the built library.
//
// The plan is what is fixed when the handle is created; the handle keeps it (rvio_hip::plan) and its launch sites read it.  WHICH kernels an update
// launches also depends on the clone count n, which grows from 0 to max_track_len - 1 while the window fills: update_forms() at the end of this file
// is the one place that decides it — the Cholesky role, the share reduction, the T product, the solve, where dx = Pc y and the state injection run,
// and the Joseph stage, each as an enum with its grid and, for every launch with dynamic LDS, the byte count and the LpKernel whose limit
// (plan.attr) covers it.  The launch functions of rvio_hip.hip switch on what it returns and rvio_hip_debug_time_kernel asks it for the forms the
// frame would get; the same sweep on the CPU checks every (window, n, batch): roles only where the Joseph launch has them, LDS within the limit.
//
// The FRONT END of a frame has its decider too: front_forms() behind update_forms().  From the plan, the handle's geometry and what is known about ONE
// call (piped or per-stage, corner list or device detector, frame number, the environment's two switches, whether the handle's queues are its own) it
// derives the call's mode (run-ahead, device-side counters, which of the buffers in rotation), every cross-queue wait and signal as a flag, the stream
// ROLE of every stage, and the form of every kernel — gray, CLAHE, pyramid, detector, cornerSubPix, KLT, RANSAC / book-keeping — with grid, workgroup
// size and dynamic LDS.  rvio_hip.hip computes that value once per call and passes it down; tests/test_launch_plan.py sweeps it on the CPU.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_HD __host__ __device__
#else
#define LP_HD
#endif

#define RVIO_MAX_LEN 32          // max Tracker.nMaxTrackingLength supported (cfg E: 31)
#define RVIO_MAX_FEATURES 4096   // max Tracker.nFeatures supported: ceil(F / 2) hand-over slots <= GRAM_MAX_FEATS
#define GRAM_MAX_FEATS 2048      // feature slots of an update (the Gram stage lists them in static LDS)
#define RVIO_LDS_LIMIT 163840    // LDS of a gfx950 CU (160 KiB): what ONE workgroup may hold, static + dynamic
#define LIT_FEATS 24             // an update handed more features than this never takes the literal path (M <= LIT_FEATS * rho_max rows)
#define LIT_RING 32              // stack rows of the literal sweep staged in LDS (two blocks of LIT_RING / 2)
#ifndef FEAT_T_SMALL
#define FEAT_T_SMALL 128     // threads of a per-feature workgroup at 6n <= 127 (same-box A/B of 64 against 128 at B = 2048: profiles/r06_feat_threads_ab.txt)
#endif
#define LIT_STAMPS 5             // phase stamps of the literal sweep (instrumented build)
#define LIT_STAMP_OFF 200        // their offset behind the second part of the [A|b] block

// ---------------------------------------------------------------- footprints (doubles) of the kernels' dynamic LDS
// feat_build_kernel, one workgroup per feature slot:
//   xcl[7*nmax] pose[(L-1)*24] hrr[L*6] hf[2L*3] lr[(L-1)*18] vh[3*2L] misc[16]
//   Hx[2L][ldh]  ([Hx | r], row-major)   Tm[rho][ldh]   S[(rho+1)][rho+1]
LP_HD inline size_t feat_lds_doubles(int max_len, int ldh, bool tm_in_lds) {
    const int L = max_len, M2 = 2 * L, rho = 2 * L - 2;
    size_t n = (size_t)7 * (L - 1) + (size_t)(L - 1) * 24 + L * 6 + M2 * 3 + (L - 1) * 18 + 3 * M2 + 16;
    n += (size_t)M2 * ldh;
    if (tm_in_lds) n += (size_t)rho * ldh;
    n += (size_t)(rho + 1) * (rho + 1);
    return n;
}
LP_HD inline int trunc_mmax(int max_len) { return 6 * ((max_len + 1) / 2 - 1); }   // largest e2 + 1
LP_HD inline size_t trunc_lds_doubles(int max_len) { const size_t m = trunc_mmax(max_len); return m * (m | 1) + m + 8; }
LP_HD inline size_t gram_batch_lds_doubles(int max_len, int ldh) {
    const size_t a = (size_t)(ldh - 1) * ldh, t = trunc_lds_doubles(max_len);
    return a > t ? a : t;
}
// state of the literal sweep's array: U (running rows), X[2] (rows in flight between cells, double-buffered), each `tri` doubles: cell n owns
// columns n..Nc (Nc = the residual), offset n (Nc + 1) - n (n - 1) / 2
LP_HD inline size_t lit_tri(int c6) { return (size_t)c6 * (c6 + 1) / 2 + c6; }
// LDS of lit_finish besides the state: ring of stack rows, (c, s) pairs of two steps, the level-to-level hand-over of two steps, row norms, the row map
LP_HD inline size_t lit_aux_doubles(int ldh, int rho_max) { return (size_t)LIT_RING * ldh + 4 * (size_t)ldh + 2 * 256 + ldh + (size_t)(LIT_FEATS * rho_max + 1) / 2 + 8; }
LP_HD inline size_t lit_state_doubles(int c6) { return 3 * lit_tri(c6); }
// a feature's raw block in LDS for the nullspace sweep: 2 max_len rows of [Hx columns + residual | Hf (3)]
LP_HD inline size_t lit_slab_doubles(int ldh, int rho_max) { return (size_t)(rho_max + 2) * (ldh + 3); }
// the export buffer: LIT_FEATS blocks of 2 max_len rows x ldh, then the Hf blocks (2 max_len x 3 each)
// + the projected blocks the nullspace sweep leaves (rho_max rows x ldh each): the raw blocks stay as exported, a second run on the same export
// (rvio_hip_debug_time_kernel) finds what the first one found
LP_HD inline size_t lit_rows_doubles(int ldh, int rho_max) { return (size_t)LIT_FEATS * (rho_max + 2) * (ldh + 3) + (size_t)LIT_FEATS * rho_max * ldh; }
// book-keeping's refill half: tfs[F] + cds[F] float2, cid_t[F] + cid_c[F] short, then one list of F float2 per wave (8-byte aligned) + a spare 16
LP_HD inline size_t book_lds_bytes(int F, int waves) { return (((size_t)20 * F + 7) & ~(size_t)7) + (size_t)waves * F * 8 + 16; }

// ---------------------------------------------------------------- diagnostics in the unused second part of the [A|b] block (2 ldh^2 doubles)
// lit_scan_gram leaves the row norms its scan saw at [ldh^2, ldh^2 + Nc), Nc <= 6n = ldh - 1; the instrumented build adds LIT_STAMPS phase stamps at
// ldh^2 + LIT_STAMP_OFF — where the block has room for them (ldh^2 >= LIT_STAMP_OFF + LIT_STAMPS: every window but max_track_len = 3).
LP_HD inline size_t lit_norm_off(int ldh) { return (size_t)ldh * ldh; }
LP_HD inline bool lit_stamp_fits(int ldh) { return (size_t)ldh * ldh + LIT_STAMP_OFF + LIT_STAMPS <= 2 * (size_t)ldh * ldh; }
LP_HD inline size_t lit_stamp_off(int ldh, int k) { return (size_t)ldh * ldh + LIT_STAMP_OFF + k; }
// one past the last double the diagnostics write (stamps: the instrumented build)
LP_HD inline size_t lit_diag_end(int ldh, bool stamps) {
    size_t e = lit_norm_off(ldh) + (size_t)(ldh - 1);
    if (stamps && lit_stamp_fits(ldh)) { const size_t s = lit_stamp_off(ldh, LIT_STAMPS - 1) + 1; if (s > e) e = s; }
    return e;
}

// ---------------------------------------------------------------- sizes the kernel files fix (bytes): rvio_hip.hip static_asserts each against its definition
#define LP_S9CHOL4_BYTES 35976       // sizeof(S9CholLds<4, 4>)   (solve9.hip)
#define LP_S9CHOL6_BYTES 44424       // sizeof(S9CholLds<6, 4>)
#define LP_S9SMALL_BYTES 160328      // sizeof(S9SmallLds)
// solve9_small_kernel's Q / R phase: the tile 4 ti + tj that wave w forms, nibble w.  Tile (ti, tj) is (4 - tj) + (4 - ti) tile products; the hardware deals
// the waves of a workgroup to the four SIMDs round-robin (wave w on SIMD w & 3), so with the natural map w -> tile w the matrix pipes carry 26 / 22 / 18 / 14
// of the 80 products.  This map gives each of them 20:  SIMD 0: tiles 0 3 12 15 (8 + 5 + 5 + 2), SIMD 1: 1 2 7 11 (7 + 6 + 4 + 3), SIMD 2: 4 8 13 14
// (7 + 6 + 4 + 3), SIMD 3: 5 6 9 10 (6 + 5 + 5 + 4)   (tests/test_solve9_qr_map.py)
#define LP_S9SMALL_QR_MAP 0xAEBF9D7C68235410ull
#define LP_PROP3_BYTES 86432         // sizeof(Prop3Lds<16>)      (filter_kernels2.hip)
#define LP_JB_TL_DOUBLES (12 * 16 * 17)                        // JB_TL_DOUBLES   (filter_kernels.hip)
#define LP_UGL_BYTES ((2 * 64 * 65 + 88 * 65 + 2 * 16 * 65) * 8)   // UGL_LDS_DOUBLES
#define LP_FNL_BYTES ((3 * 88 * 65 + 4 * 16 * 17) * 8)             // FNL_LDS_DOUBLES
#define LP_JL_BYTES ((3 * 60 * 61 + 8 * 16 * 61 + 16) * 8)         // JL_LDS_DOUBLES
#define LP_JL_THREADS 512                                          // joseph_lds_kernel's workgroup: eight waves, one tile of a strip round each
#define LP_GEMM_T_LDS_BYTES (2 * 64 * 65 * 8)                      // gemm_T_lds_kernel's operands
// imu_pose_kernel (imu_pose.hip), odom_kernel's geometry: one wave per instance, four instances per workgroup; per wave 16 words x 64 samples of LDS
#define LP_IMUP_T 256
#define LP_IMUP_WAVES (LP_IMUP_T / 64)
#define LP_IMUP_WAVE_BYTES (16 * 64 * 8)
#define LP_IMUP_LDS_BYTES (LP_IMUP_WAVES * LP_IMUP_WAVE_BYTES)
// imu_cov_kernel (imu_cov.hip): one wave per instance, one instance per workgroup.  Per sample of a chunk 16 words of the state chain + what the
// covariance step reads (six 3 x 3 blocks of dt F, dt, the 9 x 9 block of Q: 136 words), overwritten by what the record needs behind the step (the
// 12 x 12 block and the 3 x 3 velocity block: 153 words); beside them the nine rows of Phi P11 the lanes exchange (9 x 24)
#define LP_IMUC_T 64
#define LP_IMUC_CHUNK 32
#define LP_IMUC_SLOT_WORDS (16 + 153)
#define LP_IMUC_LDS_BYTES ((LP_IMUC_SLOT_WORDS * LP_IMUC_CHUNK + 216) * 8)
// aux_update_kernel<MB> (aux_update.hip): one workgroup of eight waves per instance.  MB: the row count its register arrays are unrolled for;
// the T product deals G = ceil(d / 64) row groups x aux_splits(G) column ranges over the waves (G <= 4 at d <= 24 + 6 (RVIO_MAX_LEN - 1)).
// LDS: H~ (d x MB) | T (d x (MB + 1)) | U | S, L (MB x (MB + 1) each) | 1 / d, v~ (MB each) | xi, dx (d each) | 8, where U holds the partial
// sums of T (splits x d rows), then those of S, then K and D (2 d rows)
#define LP_AUX_T 512
#define LP_AUX_MAX_ROWS 16       // RVIO_AUX_MAX_ROWS
LP_HD inline int aux_mb(int m) { return m <= 4 ? 4 : 16; }
LP_HD inline int aux_splits(int G) { return G <= 2 ? 4 : 2; }
LP_HD inline size_t aux_u_doubles(int d, int MB) {
    const int S = aux_splits((d + 63) >> 6);
    return (size_t)(S > 2 ? S : 2) * d * (MB + 1);
}
LP_HD inline size_t aux_lds_doubles(int d, int MB) {
    return (size_t)d * MB + (size_t)d * (MB + 1) + aux_u_doubles(d, MB) + 2 * (size_t)MB * (MB + 1) + 2 * MB + 2 * (size_t)d + 8;
}
// the largest footprint over the clone counts 0 .. nmax a handle passes through (not the last one's: the column ranges go from 4 to 2 at d = 129)
LP_HD inline size_t aux_lds_max_doubles(int nmax, int MB) {
    size_t w = 0;
    for (int n = 0; n <= nmax; ++n) { const size_t a = aux_lds_doubles(24 + 6 * n, MB); if (a > w) w = a; }
    return w;
}
// aux_iter_kernel<MB> (aux_update.hip), one pass of the iterated update: the same footprint + the correction of the previous pass (d doubles)
LP_HD inline size_t aux_iter_lds_doubles(int d, int MB) { return aux_lds_doubles(d, MB) + (size_t)d; }
LP_HD inline size_t aux_iter_lds_max_doubles(int nmax, int MB) {
    size_t w = 0;
    for (int n = 0; n <= nmax; ++n) { const size_t a = aux_iter_lds_doubles(24 + 6 * n, MB); if (a > w) w = a; }
    return w;
}
// the per-instance block of the iterated measurement chain (rvio_hip.hip MeasIter): doubles between the instances' snapshots — the state, then
// the pose line in the last 7 — and the block's bytes: snapshots | dx | records (rvio_meas_iter, 24 bytes) | running flags
#define LP_MEAS_MAX_ITERS 8      // RVIO_MEAS_MAX_ITERS
LP_HD inline size_t meas_iter_x0_stride(int nmax) { return (size_t)26 + 7 * (size_t)nmax + 7; }
LP_HD inline size_t meas_iter_block_bytes(int batch, int nmax, int dmax) { return (size_t)batch * (8 * meas_iter_x0_stride(nmax) + 8 * (size_t)dmax + 24 + 4); }
// standstill_kernel (standstill.hip): one workgroup of four waves per instance; the combine of the waves' partial sums goes through static LDS
// (LP_SS_RED doubles per wave), there is no dynamic part
#define LP_SS_T 256
#define LP_SS_WAVES (LP_SS_T / 64)
#define LP_SS_RED 6
// fix_rows_kernel (fix_rows.hip): ONE wave per instance; the 6 x 24 head of the Jacobian is assembled in static LDS (LP_FIX_HEAD doubles), there
// is no dynamic part
#define LP_FIX_T 64
#define LP_FIX_ROWS 6
#define LP_FIX_HEAD (LP_FIX_ROWS * 24)
// fix_past_kernel (fix_past.hip): ONE wave per instance; beside the same head, the chain of rigid transforms (A_m, t_m), m = 0 .. LP_FIXP_NMAX, from
// the reference frame back through the clone window (12 doubles each) lies in static LDS once the in-wave scan has formed it; no dynamic part
#define LP_FIXP_T 64
#define LP_FIXP_NMAX 32
#define LP_FIXP_CHAIN ((LP_FIXP_NMAX + 1) * 12)
// rel_rows_kernel (rel_rows.hip): the same wave, window limit and chain layout (LP_FIXP_T, LP_FIXP_NMAX, LP_FIXP_CHAIN) — the chain runs between two
// frames of the window instead of from the reference frame back; its rows have no head block, so the chain is all of its static LDS
// map_rows_kernel (map_rows.hip): ONE workgroup of four waves per instance.  Every wave forms the chain of fix_past_kernel (LP_FIXP_NMAX,
// LP_FIXP_CHAIN); the rows of at most LP_MAP_POINTS observed points (two each: LP_MAP_ROWS = the row limit of the auxiliary update) are staged
// TRANSPOSED in static LDS ([column][row], LP_MAP_HS doubles) for the per-point gate, whose product with P wave g forms for the g-th 64 of the
// 6 + 6 a <= LP_MAP_NZ columns that are not zero; per slot LP_MAP_SLOT doubles of geometry and LP_MAP_WAVES x 3 partial sums.  No dynamic part.
// LP_MAP_MIN_DEPTH (m): a point nearer to the camera plane than this, or behind it, is rejected — a tuning value, not a measurement.
#define LP_MAP_T 256
#define LP_MAP_WAVES (LP_MAP_T / 64)
#define LP_MAP_POINTS 8          // RVIO_MAP_MAX_POINTS
#define LP_MAP_ROWS (2 * LP_MAP_POINTS)
#define LP_MAP_DMAX (24 + 6 * LP_FIXP_NMAX)
#define LP_MAP_NZ (6 + 6 * LP_FIXP_NMAX)
#define LP_MAP_HS (LP_MAP_DMAX * LP_MAP_ROWS)
#define LP_MAP_SLOT 28           // head 2 x 6 (12) | M (6) | w (3) | r (2) | sigma (2) | depth | gamma | pad
#define LP_MAP_PART (LP_MAP_WAVES * LP_MAP_POINTS * 3)
#define LP_MAP_LDS_DOUBLES (LP_FIXP_CHAIN + LP_MAP_HS + LP_MAP_POINTS * LP_MAP_SLOT + LP_MAP_PART)
#define LP_MAP_MIN_DEPTH 0.1
static_assert(LP_MAP_ROWS == LP_AUX_MAX_ROWS, "a map call's rows fill one auxiliary update");
static_assert(LP_MAP_NZ <= 64 * LP_MAP_WAVES, "one lane per non-zero column");
// window_pose_kernel (window_pose.hip): ONE workgroup of four waves per (instance, age), grid (ages, 1, instances).  Every wave forms the chain
// of fix_past_kernel (LP_FIXP_NMAX, LP_FIXP_CHAIN); the 6 + 6 a <= LP_WINP_NZ columns of the 6-row pose Jacobian that are not zero and the
// product T = P_nz J^T lie in static LDS ([entry][6] each), beside the shares of the LP_WINP_GROUPS groups of C = J T (two orders per entry of the
// 6 x 6) and the record's words.  No dynamic part.
#define LP_WINP_T 256
#define LP_WINP_NZ (6 + 6 * LP_FIXP_NMAX)
#define LP_WINP_GROUPS 7
#define LP_WINP_WORDS 46         // sizeof(rvio_window_pose) / 8
#define LP_WINP_LDS_DOUBLES (LP_FIXP_CHAIN + 2 * 6 * LP_WINP_NZ + LP_WINP_GROUPS * 36 * 2 + LP_WINP_WORDS)
static_assert(LP_WINP_GROUPS * 36 <= LP_WINP_T, "one thread per (group, entry of the 6 x 6)");
// window_edge_kernel (window_edge.hip): ONE workgroup of four waves per (instance, pair), grid (pairs, 1, instances).  Every wave forms the local
// chain of rel_rows_kernel (LP_FIXP_NMAX, LP_FIXP_CHAIN); the 6 (b - a) <= LP_WEDGE_NZ columns of the six RVIO_REL_POSE rows that are not zero
// and the product T = P_span H^T lie in static LDS ([entry][6] each), beside the shares of the LP_WEDGE_GROUPS groups of C = H T and the record's
// words.  No dynamic part.  LP_WEDGE_MAX_PAIRS: every pair of the longest window, the most one rvio_hip_get_window_edges takes.
#define LP_WEDGE_T 256
#define LP_WEDGE_NZ (6 * LP_FIXP_NMAX)
#define LP_WEDGE_GROUPS 7
#define LP_WEDGE_WORDS 47        // sizeof(rvio_window_edge) / 8
#define LP_WEDGE_MAX_PAIRS 528   // 33 * 32 / 2
#define LP_WEDGE_LDS_DOUBLES (LP_FIXP_CHAIN + 2 * 6 * LP_WEDGE_NZ + LP_WEDGE_GROUPS * 36 * 2 + LP_WEDGE_WORDS)
static_assert(LP_WEDGE_GROUPS * 36 <= LP_WEDGE_T && LP_WEDGE_WORDS <= LP_WEDGE_T, "one thread per (group, entry of the 6 x 6) and per word");
// window_joint_kernel (window_edge.hip): ONE workgroup of four waves per (instance, age), grid (ages, 1, instances): window_pose_kernel's chain,
// J_a, T_a = P_nz J_a^T, shares and record, and beside them the staged J_b of the block in hand (b < a) and the shares of X_ba = J_b T_a (one
// order per entry: the block is not symmetric).  No dynamic part.
#define LP_WJNT_T LP_WINP_T
#define LP_WJNT_LDS_DOUBLES (LP_WINP_LDS_DOUBLES + 6 * LP_WINP_NZ + LP_WINP_GROUPS * 36)
// landmark_cov_kernel (landmark_cov.hip): ONE workgroup of four waves per (instance, cloud slot), grid (cloud slots, 1, instances).  The track's
// chain (R_i, p_i, the running rotations, the point and the lever translation at every image: LP_LMC_CHAIN doubles), the 2 x 3 blocks Hf_i and
// rho Hp_i R_ci of its at most LP_FIXP_NMAX + 1 observations, the 4 x 3 products summed per column, the LP_LMC_ROWS = 7 rows (M over {R}, M over
// the world frame, the rho row of A Hx) of the 6 + 6 nPh <= LP_LMC_NZ columns that are not zero and the product T = P_nz [rows]^T lie in static
// LDS, beside the shares of the LP_LMC_GROUPS groups of the LP_LMC_ENTS = 9 + 9 + 1 entries (two orders each) and the record's words.  The
// 2 L x 6 nPh Jacobian Hx is never stored.  No dynamic part.  LP_LMC_PIVOT_EPS: a Cholesky pivot of N at or below this share of its diagonal
// entry counts as not positive (status 1): 2 L_max rounding errors of the sum that forms the entry.
#define LP_LMC_T 256
#define LP_LMC_LMAX (LP_FIXP_NMAX + 1)
#define LP_LMC_NZ (6 + 6 * LP_FIXP_NMAX)
#define LP_LMC_ROWS 7
#define LP_LMC_GROUPS 13
#define LP_LMC_ENTS 19
#define LP_LMC_WORDS 28          // sizeof(rvio_landmark_cov) / 8
#define LP_LMC_PIVOT_EPS (64 * 2.220446049250313e-16)
#define LP_LMC_CHAIN (LP_FIXP_NMAX * 12 + LP_LMC_LMAX * 15)
#define LP_LMC_LDS_DOUBLES (LP_LMC_CHAIN + LP_LMC_LMAX * 24 + 2 * LP_LMC_ROWS * LP_LMC_NZ + LP_LMC_GROUPS * LP_LMC_ENTS * 2 + 96 + LP_LMC_WORDS)
static_assert(LP_LMC_GROUPS * LP_LMC_ENTS <= LP_LMC_T && LP_LMC_NZ <= LP_LMC_T && LP_LMC_WORDS <= LP_LMC_T, "one thread per (group, entry), per non-zero column and per word");
// doubles between the instances' rows in the block of the map calls, and that block's bytes: rows | r | sigma | (gamma, applied) | records |
// per-slot records | flags
LP_HD inline size_t map_H_stride(int dmax) { return (size_t)LP_MAP_ROWS * dmax; }
LP_HD inline size_t map_block_bytes(int batch, int dmax) {
    return (size_t)batch * (8 * map_H_stride(dmax) + 8 * LP_MAP_ROWS + 8 * LP_MAP_ROWS + 16 + 32 + 40 * LP_MAP_POINTS + 4);
}

// ---------------------------------------------------------------- the kernels create_impl gives a dynamic-LDS limit
enum LpKernel {
    LPK_FEAT_BUILD16, LPK_FEAT_BUILD4, LPK_GRAM_REDUCE, LPK_BLOCK_SUM, LPK_LIT_BATCH, LPK_GEMM_T_LDS, LPK_GRAM_BATCH4, LPK_GRAM_BATCH6, LPK_FEAT_PROP,
    LPK_BOOKKEEP_B, LPK_RANSAC_BOOK, LPK_SOLVE9_SMALL, LPK_SOLVE6_1, LPK_SOLVE6_2, LPK_SOLVE6_3, LPK_JOSEPH_BATCH, LPK_UG, LPK_UG_LDS, LPK_FINAL_LDS,
    LPK_JOSEPH_LDS, LPK_IMU_POSE, LPK_AUX_UPDATE4, LPK_AUX_UPDATE16, LPK_IMU_COV, LPK_STANDSTILL, LPK_FIX, LPK_FIX_PAST, LPK_REL, LPK_MAP,
    LPK_AUX_ITER4, LPK_AUX_ITER16, LPK_WINDOW_EDGE, LPK_WINDOW_JOINT, LPK_LANDMARK_COV, LPK_WINDOW_POSE, LPK_COUNT
};
// (as c++filt prints them, without return type and arguments: how the test finds each kernel's static LDS in the code object's notes)
static const char* const kLpKernelName[LPK_COUNT] = {
    "feat_build_kernel<16>", "feat_build_kernel<4>", "gram_reduce_kernel", "block_sum_kernel", "lit_batch_kernel", "gemm_T_lds_kernel",
    "gram_reduce_batch_kernel<4>", "gram_reduce_batch_kernel<6>", "feat_prop_kernel", "bookkeep_b_kernel", "ransac_book_kernel", "solve9_small_kernel",
    "solve6_kernel<1, 8, 8>", "solve6_kernel<2, 12, 8>", "solve6_kernel<2, 16, 8>", "joseph_batch_kernel", "ug_kernel", "ug_lds_kernel", "final_lds_kernel",
    "joseph_lds_kernel", "imu_pose_kernel", "aux_update_kernel<4>", "aux_update_kernel<16>", "imu_cov_kernel", "standstill_kernel",
    "fix_rows_kernel", "fix_past_kernel", "rel_rows_kernel", "map_rows_kernel", "aux_iter_kernel<4>", "aux_iter_kernel<16>", "window_edge_kernel",
    "window_joint_kernel", "landmark_cov_kernel", "window_pose_kernel"
};

struct LaunchPlan {
    int rc = 0;                  // 0, or 1: the configuration is not supported (why says which limit)
    const char* why = nullptr;
    int Fu = 0, ldh = 0, rho_max = 0;
    int feat_threads = 256;
    int n_ic = 2;                // image chains in flight
    bool chol_queue = false;     // long windows (96 < 6n <= 192, one instance): the queue a second image chain would take runs the Cholesky factor of the clone block
    size_t trunc_lds = 0, lit_batch_lds = 0, feat_lds = 0, fprop_lds = 0, gram_batch_lds = 0, book_lds = 0, solve5_lds = 0, jb_lds = 0, ug_lds = 0;
    bool lit_state_global = false, tm_global = false, fuse_ok = false;
    bool lit_ok = false;         // the window admits the literal sweep (literal.h): its row / rotation tables and one raw feature block fit where they are staged
    int book_waves = 4;
    bool book_fused = false;     // RANSAC + both halves of book-keeping in one launch (ransac_book_kernel) fit one CU; else ransac_book_a_kernel + bookkeep_b_kernel
    int solve5_variant = 0, solve7_variant = 0, solve9_nt = 0;
    size_t attr[LPK_COUNT] = {}; // dynamic-LDS limit to set per kernel (0: none)
};

LP_HD inline size_t lp_max(size_t a, size_t b) { return a > b ? a : b; }
LP_HD inline size_t lp_min(size_t a, size_t b) { return a < b ? a : b; }

// statics[k]: static LDS (bytes) of kernel k of THIS build
inline LaunchPlan launch_plan(int max_len, int n_features, int batch, const size_t* statics) {
    LaunchPlan p;
    const int nmax = max_len - 1;
    p.Fu = (n_features + 1) / 2; p.ldh = 6 * nmax + 1; p.rho_max = 2 * max_len - 2;
    const size_t ldh = p.ldh, c6m = ldh - 1;
    const int F = n_features;
    if (max_len < 3 || max_len > RVIO_MAX_LEN || n_features < 2 || batch < 1) { p.rc = 1; p.why = "invalid configuration"; return p; }
    if (p.Fu > GRAM_MAX_FEATS) { p.rc = 1; p.why = "Tracker.nFeatures too large: at most 4096 (RVIO_MAX_FEATURES; ceil(F/2) hand-over slots <= 2048 in the Gram stage)"; return p; }
    // Image chains in flight.  Two (default): with the filter, tracker and side streams that makes FOUR busy queues.  Long windows
    // (96 < 6n <= 192: the solve in its split form, filter chain >= 250 us): ONE image chain in flight is enough (the chain is ~180 us),
    // and the queue that frees runs the Cholesky factor of the clone block beside the filter chain.
    if (batch == 1 && c6m > 96 && c6m <= 192) { p.n_ic = 1; p.chol_queue = true; }
    p.feat_threads = (p.ldh <= 128) ? FEAT_T_SMALL : 256;
    p.lit_ok = p.ldh <= 190 && nmax + 1 <= 40 && p.rho_max < 254 && lit_slab_doubles(p.ldh, p.rho_max) * sizeof(double) <= 144 * 1024;
    p.trunc_lds = trunc_lds_doubles(max_len) * sizeof(double);
    {   // the literal sweep runs in the workgroup that finishes the reduction (literal.h): its ring / rotation tables always in that launch's LDS, the
        // array's state too when it fits beside gram_reduce_kernel's static LDS — else, and for batch handles (occupancy), in the slab
        const size_t aux = lit_aux_doubles(p.ldh, p.rho_max) * sizeof(double), st = lit_state_doubles(p.ldh - 1) * sizeof(double);
        const size_t slab = lit_slab_doubles(p.ldh, p.rho_max) * sizeof(double);   // (a feature's raw block for the nullspace sweep: at least one must fit)
        p.lit_state_global = batch > 1 || aux + st > 144 * 1024;
        p.lit_batch_lds = lp_max(aux, slab);
        p.trunc_lds = lp_max(p.trunc_lds, lp_max(p.lit_state_global ? aux : aux + st, lp_min((size_t)4, (size_t)(144 * 1024) / slab) * slab));
    }
    p.feat_lds = feat_lds_doubles(max_len, p.ldh, true) * sizeof(double);
    // (a batch handle keeps T in global memory as well: a third less LDS per feature workgroup = 8 instead of 5 resident per CU)
    if (p.feat_lds > 150 * 1024 || batch > 1) {
        p.feat_lds = feat_lds_doubles(max_len, p.ldh, false) * sizeof(double);
        p.tm_global = true;
    }
    if (p.feat_lds > 160 * 1024) { p.rc = 1; p.why = "per-feature LDS footprint exceeds 160 KiB"; return p; }
    p.attr[LPK_FEAT_BUILD16] = p.attr[LPK_FEAT_BUILD4] = p.feat_lds;
    p.attr[LPK_GRAM_REDUCE] = p.attr[LPK_BLOCK_SUM] = p.trunc_lds;
    p.attr[LPK_LIT_BATCH] = p.lit_batch_lds;
    if (batch > 1 && gram_batch_lds_doubles(max_len, p.ldh) * sizeof(double) <= 64 * 1024) {
        p.gram_batch_lds = gram_batch_lds_doubles(max_len, p.ldh) * sizeof(double);
        p.attr[LPK_GEMM_T_LDS] = LP_GEMM_T_LDS_BYTES;
        p.attr[LPK_GRAM_BATCH4] = p.attr[LPK_GRAM_BATCH6] = p.gram_batch_lds;
    }
    // propagate rides in the per-feature launch: its workgroup builds no feature, so its buffers (Prop3Lds<16>, 86 KB) and the per-feature footprint
    // share the launch's dynamic LDS — max of the two, which fits one CU for every window (rounds 2-4: static + dynamic, the SUM: long windows
    // fell back to 8-sample chunks, cfg E to a propagate launch of its own on the chain)
    p.fprop_lds = p.feat_lds;
    // (round 5: + the Cholesky role of solve9 at 6n <= 96 — one more workgroup whose buffers live in the launch's dynamic LDS too)
    if (batch == 1 && c6m <= 96) p.fprop_lds = lp_max(p.fprop_lds, c6m <= 64 ? (size_t)LP_S9CHOL4_BYTES : (size_t)LP_S9CHOL6_BYTES);
    p.fprop_lds = lp_max(p.fprop_lds, (size_t)LP_PROP3_BYTES);
    p.fuse_ok = batch == 1 && p.fprop_lds + statics[LPK_FEAT_PROP] <= RVIO_LDS_LIMIT;
    if (p.fuse_ok) p.attr[LPK_FEAT_PROP] = p.fprop_lds;
    // the refill half of book-keeping walks the ChessGrid one wave per cell with a per-wave list of the cell's points (F float2 each): as many
    // waves as one CU's LDS holds BESIDE THE KERNEL'S STATIC LDS for one stream (16 at F <= 1001: 20 cells -> two rounds instead of five), 4 for
    // batch handles (occupancy).  The fused launch (RANSAC + both halves, ransac_book_kernel: ~15 KB static, >= 4 waves — RANSAC's inlier count
    // needs 256 threads) where that fits; beyond it (F >= 2851) the pair ransac_book_a_kernel + bookkeep_b_kernel, whose refill half has
    // next to no static LDS and runs with any number of waves.
    {
        const int top = batch == 1 ? 16 : 4;
        for (int nwv = top; nwv >= 4 && !p.book_fused; nwv /= 2)
            if (book_lds_bytes(F, nwv) + lp_max(statics[LPK_RANSAC_BOOK], statics[LPK_BOOKKEEP_B]) <= RVIO_LDS_LIMIT) { p.book_waves = nwv; p.book_fused = true; }
        if (!p.book_fused) {
            p.book_waves = 0;
            for (int nwv = top; nwv >= 1 && !p.book_waves; nwv /= 2)
                if (book_lds_bytes(F, nwv) + statics[LPK_BOOKKEEP_B] <= RVIO_LDS_LIMIT) p.book_waves = nwv;
            if (!p.book_waves) { p.rc = 1; p.why = "Tracker.nFeatures too large for book-keeping's LDS lists (160 KiB per workgroup)"; return p; }
        }
        p.book_lds = book_lds_bytes(F, p.book_waves);
        p.attr[LPK_BOOKKEEP_B] = p.book_lds;
        if (p.book_fused) p.attr[LPK_RANSAC_BOOK] = p.book_lds;
    }
    {   // solve6_kernel (the LDS-tableau solve behind gemm_T_kernel): variants <column chunks, rows per wave> for c6 <= 126
        int rpw = 0, nch = 0;
        const int nw = 8;
        if (c6m <= 60) { p.solve5_variant = 1; nch = 1; rpw = 8; }
        else if (c6m <= 96) { p.solve5_variant = 2; nch = 2; rpw = 12; }
        else if (c6m <= 126) { p.solve5_variant = 3; nch = 2; rpw = 16; }
        // one instance: the blocked SPD solve (solve9.hip).  Measured on full-load updates (tools/solve9_probe.py, profiles/r05_solve9_probe.txt), solve kernel alone,
        // against the register-tableau elimination of rounds 3-4: 6n = 84: 94.0 us against 102.6; 120: 173 against 212; 180: 511 against 797.  At 6n <= 96 the Cholesky
        // of the clone block — the part that does not depend on the measurements — rides as one more workgroup in the per-feature launch (pipelined frame) or in
        // propagate's launch (staged entry points), off the chain; the solve kernel then starts at Q = A L.
        if (batch == 1 && c6m <= 192) {
            p.solve9_nt = (c6m <= 64) ? 4 : (c6m <= 96) ? 6 : (c6m <= 128) ? 8 : 12;
            if (p.solve9_nt == 4) p.attr[LPK_SOLVE9_SMALL] = LP_S9SMALL_BYTES;
        }
        // batch handles: throughput, not latency — solve6 keeps four instances resident per CU (33 KB of LDS against 112 KB) and the
        // multi-workgroup gemm_T_kernel costs nothing there (measured at B = 2048: 2.67 ms per batched frame against 3.09)
        // (round 3, measured and NOT adopted: the register-tableau solve with T through the L2 scratch instead of LDS — 11 KB of LDS, eight workgroups per CU, no
        // gemm_T launch — as the batch form at 6n <= 64: 2.62 ms per batched frame at B = 2048 against 2.29 with solve6 behind gemm_T)
        // ... and beyond solve6's windows (126 < 6n <= 192) the register-tableau solve with the T prologue: solve7_kernel<3, 16, 12>
        if (batch > 1 && !p.solve5_variant && c6m <= 192) p.solve7_variant = 4;
        if (p.solve5_variant) {
            p.solve5_lds = (size_t)(nw * rpw) * (64 * nch + 1) * sizeof(double);
            p.attr[LPK_SOLVE6_1] = p.attr[LPK_SOLVE6_2] = p.attr[LPK_SOLVE6_3] = lp_max(p.solve5_lds, (size_t)1024);
        }
    }
    const size_t c6t = (c6m + 15) / 16;
    if (batch >= 128 && c6m <= 60) {   // the Joseph form of a batch handle in one kernel, one workgroup per instance
        const size_t ls = c6m + 1, dmx = 24 + c6m;
        p.jb_lds = (3 * dmx * ls + lp_max(c6m * ls, (size_t)LP_JB_TL_DOUBLES)) * sizeof(double);
        if (p.jb_lds + statics[LPK_JOSEPH_BATCH] > RVIO_LDS_LIMIT) p.jb_lds = 0;
        else p.attr[LPK_JOSEPH_BATCH] = p.jb_lds;
    }
    p.ug_lds = 2 * 16 * (c6t * 16 + 1) * sizeof(double);
    p.attr[LPK_UG] = p.ug_lds;
    p.attr[LPK_UG_LDS] = LP_UGL_BYTES;
    p.attr[LPK_FINAL_LDS] = LP_FNL_BYTES;
    p.attr[LPK_JOSEPH_LDS] = LP_JL_BYTES;
    p.attr[LPK_IMU_POSE] = LP_IMUP_LDS_BYTES;
    p.attr[LPK_IMU_COV] = LP_IMUC_LDS_BYTES;
    p.attr[LPK_AUX_UPDATE4] = aux_lds_max_doubles(nmax, 4) * sizeof(double);      // (what a launch asks for follows the clone count)
    p.attr[LPK_AUX_UPDATE16] = aux_lds_max_doubles(nmax, 16) * sizeof(double);
    p.attr[LPK_AUX_ITER4] = aux_iter_lds_max_doubles(nmax, 4) * sizeof(double);
    p.attr[LPK_AUX_ITER16] = aux_iter_lds_max_doubles(nmax, 16) * sizeof(double);
    // standstill_kernel asks for no dynamic LDS (p.attr[LPK_STANDSTILL] stays 0: no limit to set); its static part alone is held to a CU here
    if (statics[LPK_STANDSTILL] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // fix_rows_kernel: the same (static LDS only, p.attr[LPK_FIX] stays 0)
    if (statics[LPK_FIX] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // fix_past_kernel: likewise (p.attr[LPK_FIX_PAST] stays 0)
    if (statics[LPK_FIX_PAST] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // rel_rows_kernel: likewise (p.attr[LPK_REL] stays 0)
    if (statics[LPK_REL] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // map_rows_kernel: likewise (p.attr[LPK_MAP] stays 0)
    if (statics[LPK_MAP] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // window_edge_kernel, window_joint_kernel: likewise (their p.attr stay 0)
    if (statics[LPK_WINDOW_EDGE] > RVIO_LDS_LIMIT || statics[LPK_WINDOW_JOINT] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // landmark_cov_kernel: likewise (p.attr[LPK_LANDMARK_COV] stays 0)
    if (statics[LPK_LANDMARK_COV] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    // window_pose_kernel: likewise (p.attr[LPK_WINDOW_POSE] stays 0)
    if (statics[LPK_WINDOW_POSE] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    if (batch > 1 && !p.solve5_variant && !p.solve7_variant) { p.rc = 1; p.why = "batched filter: clone window too long for the unrolled solve kernel (6n <= 126)"; return p; }
    // nothing above may ask for more than a CU has: a configuration that would is refused here, by name, not by a failed hipFuncSetAttribute / launch
    for (int k = 0; k < LPK_COUNT; ++k)
        if (p.attr[k] && p.attr[k] + statics[k] > RVIO_LDS_LIMIT) { p.rc = 1; p.why = "LDS footprint (static + dynamic) of a kernel exceeds the 160 KiB of a CU"; return p; }
    return p;
}

// ---------------------------------------------------------------- the forms of ONE update: what depends on the clone count n as well
enum LpChol {            // who factors the clone block Pcc = L L^T ahead of the solve
    LPC_NONE,            //   nobody: the solve does it (batch handles; n = 0)
    LPC_ROLE,            //   6n_max <= 96: one more workgroup of feat_prop_kernel (pipelined frame) or of propagate_chol_kernel<2|3> (staged entry points)
    LPC_QUEUE            //   6n_max > 96: solve9_chol_kernel on the queue plan.chol_queue frees, started behind augment / compose
};
enum LpGram { LPG_REDUCE, LPG_BATCH4, LPG_BATCH6 };   // gram_reduce_kernel, gram_reduce_batch_kernel<4>, <6>
enum LpTprod { LPT_NONE, LPT_GEMM, LPT_GEMM_LDS };    // no launch (the solve forms T itself), gemm_T_kernel, gemm_T_lds_kernel
enum LpSolve {
    LPS_NONE, LPS_SMALL, LPS_S9_1_4, LPS_S9_2_3, LPS_S9_2_3_PRE,   // solve9_small_kernel, solve9_kernel<1, 4>, <2, 3>, <2, 3, true>
    LPS_SPLIT,                                                      // the split form: solve9_prod / _sweep launches at split_nt = 8 | 12, behind a solve9_chol launch if own_chol
    LPS_SOLVE7, LPS_SOLVE6_1, LPS_SOLVE6_2, LPS_SOLVE6_3            // solve7_kernel<3, 16, 12>, solve6_kernel<1, 8, 8>, <2, 12, 8>, <2, 16, 8>
};
enum LpDx { LPD_INSIDE, LPD_KERNEL, LPD_ROLES };   // dx = Pc y and the state injection: in the solve kernel, a solve9_dx_kernel launch, role workgroups of the Joseph launch
enum LpJoseph {
    LPJ_BATCH,       // joseph_batch_kernel                                     grid[0]
    LPJ_LDS,         // joseph_lds_kernel (has roles)                           grid[0]
    LPJ_LDS_PAIR,    // ug_lds_kernel, final_lds_kernel                         grid[0], grid[1]
    LPJ_TILE,        // ug_tile_kernel<0> (has roles), <1>, <2>, final_tile_kernel   grid[0..3]
    LPJ_STRIPS       // ug_kernel, final_kernel                                 grid[0], grid[1]
};
struct LpLds { size_t bytes = 0; int kernel = -1; };   // dynamic LDS of one launch, and the LpKernel whose limit (plan.attr) covers it; kernel < 0: the launch has none

struct UpdateForms {
    LpChol chol = LPC_NONE;
    LpGram gram = LPG_REDUCE;
    int gram_grid = 1;           // workgroups per instance
    bool gram_finish = false;    // gram_reduce_kernel: the last workgroup turns the block into [A|b] (the batch kernels always do)
    bool lit_batch = false;      // lit_batch_kernel follows the batch reduction
    LpLds gram_lds, lit_lds;
    LpTprod tprod = LPT_NONE;
    int tprod_grid = 0;          // gemm_T_kernel: tprod_grid x tprod_grid workgroups per instance
    LpLds tprod_lds;
    LpSolve solve = LPS_NONE;
    int split_nt = 0;
    bool own_chol = false;
    LpLds solve_lds;
    LpDx dx = LPD_INSIDE;
    LpJoseph joseph = LPJ_STRIPS;
    int grid[4] = {0, 0, 0, 0};  // workgroups per instance of the Joseph stage's launches, WITHOUT the roles
    int role_wgs = 0;            // dx == LPD_ROLES: workgroups added to the first Joseph launch
    LpLds ug_lds, fin_lds;       // of the first (or only) Joseph launch, and of final_lds_kernel
};

// plan: of this handle; batch: its instances; n: clones in the window now; pre: a factor of the clone block is in the slab already (or in flight on
// the Cholesky queue); whole_update: the solve with both Joseph stages right behind it (else: one separately timed stage); combined: the unsharded
// update (world == 1, the reduction finishes into [A|b]); lit: the handle has the literal path's buffers.
// A branch that no handle can reach is kept and marked.
inline UpdateForms update_forms(const LaunchPlan& p, int batch, int n, bool pre, bool whole_update, bool combined, bool lit) {
    UpdateForms f;
    const int B = batch, c6 = 6 * n, dd = 24 + c6, NT = p.solve9_nt;
    const int nt = (dd + 15) / 16, npair = nt * (nt + 1) / 2;
    // the Cholesky of the clone block: it does not depend on the measurements, so it runs off the chain
    if (NT && NT <= 6 && n >= 1) f.chol = LPC_ROLE;
    else if (NT >= 8 && p.chol_queue && n >= 1) f.chol = LPC_QUEUE;
    // the share reduction.  A batch handle whose [A|b] fits in LDS (6n <= 90): one workgroup per instance, tiles of 16, 4 x 4 up to 6n = 63, 6 x 6 beyond;
    // else 64 elements per workgroup for one stream (the shares are remote reads: spread them over many CUs), 256 for a batch (fewer, fuller workgroups)
    if (B >= 128 && combined && p.gram_batch_lds) {
        const bool four = p.ldh - 1 <= 63;
        f.gram = four ? LPG_BATCH4 : LPG_BATCH6;
        f.gram_lds = {p.gram_batch_lds, four ? LPK_GRAM_BATCH4 : LPK_GRAM_BATCH6};
        f.lit_batch = lit;
        if (lit) f.lit_lds = {p.lit_batch_lds, LPK_LIT_BATCH};
    } else {
        const int chunk = (B == 1) ? 64 : 256, want = (6 * n * p.ldh + chunk - 1) / chunk;
        f.gram_grid = want > 1024 ? 1024 : want < 1 ? 1 : want;
        f.gram_finish = combined;
        f.gram_lds = {p.trunc_lds, LPK_GRAM_REDUCE};
    }
    // T = s2 I + A Pcc as a launch of its own: for the solves that do not form it themselves (solve6: batch handles up to 6n = 126)
    if (!p.solve7_variant && !NT) {
        if (B >= 128 && p.ldh - 1 <= 64) { f.tprod = LPT_GEMM_LDS; f.tprod_lds = {(size_t)2 * c6 * (c6 + 1) * sizeof(double), LPK_GEMM_T_LDS}; }
        else { f.tprod = LPT_GEMM; f.tprod_grid = (c6 + 31) / 32; }
    }
    // the solve
    if (NT == 4) {          // 6n <= 60: in a whole update joseph_lds_kernel follows, whose role workgroups take dx over from the all-LDS solve
        if (pre) { f.solve = LPS_SMALL; f.solve_lds = {LP_S9SMALL_BYTES, LPK_SOLVE9_SMALL}; f.dx = whole_update ? LPD_ROLES : LPD_INSIDE; }
        else f.solve = LPS_S9_1_4;
    } else if (NT == 6) {   // 64 < 6n_max <= 96: roles of joseph_lds_kernel while the window holds <= 10 clones, of ug_tile_kernel<0> from 11 on
        f.solve = pre ? LPS_S9_2_3_PRE : LPS_S9_2_3;
        f.dx = whole_update ? LPD_ROLES : LPD_INSIDE;
    } else if (NT) {        // 6n_max > 96: the split form — the product phases fill the chip, the two factorisations are one workgroup each
        f.solve = LPS_SPLIT; f.split_nt = NT; f.own_chol = !pre;
        f.dx = (whole_update && c6 > 64) ? LPD_ROLES : LPD_KERNEL;   // (6n <= 64 while the window fills: the Joseph stage takes its short-window kernels)
    }
    else if (p.solve7_variant == 4) f.solve = LPS_SOLVE7;
    else if (p.solve5_variant == 1) { f.solve = LPS_SOLVE6_1; f.solve_lds = {p.solve5_lds, LPK_SOLVE6_1}; }
    else if (p.solve5_variant == 2) { f.solve = LPS_SOLVE6_2; f.solve_lds = {p.solve5_lds, LPK_SOLVE6_2}; }
    else if (p.solve5_variant == 3) { f.solve = LPS_SOLVE6_3; f.solve_lds = {p.solve5_lds, LPK_SOLVE6_3}; }
    // the Joseph stage: U = Pc W, G = U A, P1 = (I - KH) P, then P+ = sym(P1 - P1c G^T + s2 G U^T)
    if (p.jb_lds && whole_update) {   // batch handle, 6n <= 60: P -> P+ in one kernel (U, G, P1 never leave the CU)
        f.joseph = LPJ_BATCH; f.grid[0] = 1; f.ug_lds = {p.jb_lds, LPK_JOSEPH_BATCH};
    } else if (B == 1 && c6 <= 60 && whole_update) {   // one instance, short window: both stages in ONE launch, a workgroup per tile pair of P+
        f.joseph = LPJ_LDS; f.grid[0] = npair; f.ug_lds = {LP_JL_BYTES, LPK_JOSEPH_LDS};
    } else if (B == 1 && c6 <= 64) {   // ... one stage at a time: every operand of a workgroup staged in LDS with one batch of loads.  It has no roles and
        // needs none: no window has 60 < 6n <= 64, so a whole update never gets here (unreachable with whole_update; the sweep of tests/test_launch_plan.py holds it to that)
        f.joseph = LPJ_LDS_PAIR; f.grid[0] = nt; f.grid[1] = (npair + 3) / 4;
        f.ug_lds = {LP_UGL_BYTES, LPK_UG_LDS}; f.fin_lds = {LP_FNL_BYTES, LPK_FINAL_LDS};
    } else if (B == 1) {   // one instance, 6n > 64: one wave per output tile, the chip is this instance's alone
        const int c6t = (c6 + 15) / 16;
        f.joseph = LPJ_TILE; f.grid[0] = f.grid[1] = (nt * c6t + 3) / 4; f.grid[2] = (nt * nt + 3) / 4; f.grid[3] = npair;
    } else {   // batch handles
        f.joseph = LPJ_STRIPS; f.grid[0] = (dd + 15) / 16; f.grid[1] = (npair + 3) / 4; f.ug_lds = {p.ug_lds, LPK_UG};
    }
    if (f.dx == LPD_ROLES) f.role_wgs = (dd + 23) / 24;
    return f;
}

// ---------------------------------------------------------------- the forms of ONE front-end call: mode, synchronisation, stream roles, kernel forms
// What a front-end call launches, and how its chains are ordered against each other, follows from values known when the call is made: front_forms()
// is the one place that derives them.  track_dev_impl / frame_dev_impl / rvio_hip_frame (rvio_hip.hip) compute ONE FrontForms per call and hand that
// value down to every stage; the stages switch on its enums and take grids and LDS from it.  Stream and event OBJECTS stay in rvio_hip.hip
// (stream_of maps a role to the handle's stream).
//
// sizes the front-end kernel files fix: rvio_hip.hip static_asserts each against its definition (detector.hip, clahe.hip, pyr_sep.h)
#define LP_DET_TW 64              // DET_TW: tile of the detector's fused first pass, columns
#define LP_DET_FH 16              // DET_FH: ... rows
#define LP_DET_T 512              // DET_T
#define LP_DET_SW 60              // DET_SW: strip of the throughput form, columns a wave owns
#define LP_DET_SH 16              // DET_SH: ... rows it walks
#define LP_NEIGH_T 1024           // NEIGH_T
#define LP_NEIGH_BLOCKS 8         // NEIGH_BLOCKS
#define LP_NEIGH_BLOCKS_WIDE 2    // NEIGH_BLOCKS_WIDE
#define LP_NEIGH_LDS 53256        // NEIGH_LDS
#define LP_GREEDY_T 1024          // GREEDY_T
#define LP_GREEDY_LDS 122896      // GREEDY_LDS
#define LP_SP_WIN 7               // SP_WIN: the stock cornerSubPix half-window (Tracker.nMinDist = 15)
#define LP_SP_T 256               // SP_T
#define LP_SPG_T 256              // SPG_T
#define LP_SPW_C 16               // SPW_C
#define LP_PYR_T 256              // PYR_T
#define LP_CLAHE_LUT_T 1024       // CLAHE_LUT_T
// dynamic LDS of subpix_wide_kernel for a half-window (detector.hip subpix_wide_lds: the summation grid in two sizes)
LP_HD inline size_t lp_subpix_wide_lds(int win) {
    const int G = 2 * win + 1 <= 64 ? 64 : 128;
    return sizeof(double) * ((size_t)5 * G * (LP_SPW_C + 1) + 5 * G + 8);
}

// who covers the dynamic LDS of a front-end launch (LpLaunch::kernel) when it is not a kernel of plan.attr
enum {
    LPF_NONE = -1,          // the launch has none
    LPF_DEFAULT = -2,       // no limit is set for the kernel: within the 64 KiB any kernel may ask for (RANSAC's 8 F + 16 <= 32 784 at F <= 4096)
    LPF_NEIGH = -3,         // LP_NEIGH_LDS   (detector_init sets it)
    LPF_GREEDY = -4,        // LP_GREEDY_LDS  (detector_init sets it)
    LPF_SUBPIX_WIDE = -5    // lp_subpix_wide_lds(half-window)   (detector_init sets it)
};
struct LpLaunch { int gx = 0, gy = 1, gz = 1, threads = 0; size_t lds = 0; int kernel = LPF_NONE; };   // gx == 0: not launched
// imu_pose_kernel on `instances` instances (rvio_hip_predict: one; rvio_hip_predict_dev and the IMU-rate ring: the handle's batch)
LP_HD inline LpLaunch imu_pose_launch(int instances) { return {(instances + LP_IMUP_WAVES - 1) / LP_IMUP_WAVES, 1, 1, LP_IMUP_T, LP_IMUP_LDS_BYTES, LPK_IMU_POSE}; }
// imu_cov_kernel on `instances` instances, next to imu_pose_kernel wherever that runs with covariances asked for
LP_HD inline LpLaunch imu_cov_launch(int instances) { return {instances, 1, 1, LP_IMUC_T, LP_IMUC_LDS_BYTES, LPK_IMU_COV}; }
// aux_update_kernel on a window of n clones, m rows: ONE form at every batch size (a batch handle's instance and a plain handle compute the same
// bits), the kernel instance by the row count, the dynamic LDS by the window as it is now
LP_HD inline LpLaunch aux_update_launch(int n, int m, int batch) {
    const int MB = aux_mb(m);
    return {1, 1, batch, LP_AUX_T, aux_lds_doubles(24 + 6 * n, MB) * sizeof(double), MB == 4 ? LPK_AUX_UPDATE4 : LPK_AUX_UPDATE16};
}
// aux_iter_kernel: the same grid and form choice, d more doubles of LDS
LP_HD inline LpLaunch aux_iter_launch(int n, int m, int batch) {
    const int MB = aux_mb(m);
    return {1, 1, batch, LP_AUX_T, aux_iter_lds_doubles(24 + 6 * n, MB) * sizeof(double), MB == 4 ? LPK_AUX_ITER4 : LPK_AUX_ITER16};
}
// standstill_kernel: one workgroup per instance at every batch size, static LDS only
LP_HD inline LpLaunch standstill_launch(int batch) { return {1, 1, batch, LP_SS_T, 0, LPK_STANDSTILL}; }
// fix_rows_kernel: one wave per instance at every batch size, static LDS only
LP_HD inline LpLaunch fix_launch(int batch) { return {1, 1, batch, LP_FIX_T, 0, LPK_FIX}; }
// fix_past_kernel: the same form
LP_HD inline LpLaunch fix_past_launch(int batch) { return {1, 1, batch, LP_FIXP_T, 0, LPK_FIX_PAST}; }
// rel_rows_kernel: the same form
LP_HD inline LpLaunch rel_launch(int batch) { return {1, 1, batch, LP_FIXP_T, 0, LPK_REL}; }
// map_rows_kernel: one workgroup of LP_MAP_WAVES waves per instance, static LDS only
LP_HD inline LpLaunch map_launch(int batch) { return {1, 1, batch, LP_MAP_T, 0, LPK_MAP}; }
// window_pose_kernel: one workgroup of four waves per (instance, age), static LDS only
LP_HD inline LpLaunch window_pose_launch(int batch, int n_ages) { return {n_ages, 1, batch, LP_WINP_T, 0, LPK_WINDOW_POSE}; }
// window_edge_kernel: one workgroup of four waves per (instance, pair), static LDS only
LP_HD inline LpLaunch window_edge_launch(int batch, int n_pairs) { return {n_pairs, 1, batch, LP_WEDGE_T, 0, LPK_WINDOW_EDGE}; }
// window_joint_kernel: one workgroup of four waves per (instance, age), static LDS only
LP_HD inline LpLaunch window_joint_launch(int batch, int n_ages) { return {n_ages, 1, batch, LP_WJNT_T, 0, LPK_WINDOW_JOINT}; }
// landmark_cov_kernel: one workgroup per (instance, cloud slot); the slots at and beyond the cloud's count return at once
LP_HD inline LpLaunch landmark_cov_launch(int batch, int slots) { return {slots, 1, batch, LP_LMC_T, 0, LPK_LANDMARK_COV}; }

enum LpStream {          // the ROLE of a stream in a call; stream_of (rvio_hip.hip) maps it to one of the handle's four
    LPR_FILTER,          //   the filter stream: every launch of a per-stage call that is not forked to the side stream
    LPR_TRACKER,         //   the tracker stream of the pipelined whole-frame path
    LPR_SIDE,            //   the side stream: pyramid / KLT / RANSAC beside the detector; book-keeping too in run-ahead mode
    LPR_IMAGE            //   run-ahead mode: the image chain `ic` of this frame (chain 0 shares the tracker stream's queue, chain 1 has the fourth)
};
enum LpGray {
    LPGR_NONE, LPGR_DWORD3, LPGR_BYTE3, LPGR_DWORD4, LPGR_BYTE4,   // mono: no launch; gray_kernel4<3>, gray_kernel<3>, gray_kernel4<4>, gray_kernel<4>
    // raw sensor data (raw.hip), each family in its wide form (aligned dword loads, four pixels per lane) and its plain form:
    LPGR_W16_1, LPGR_P16_1, LPGR_W16_3, LPGR_P16_3, LPGR_W16_4, LPGR_P16_4,   // 16-bit samples: raw16_kernel4<1|3|4>, raw16_kernel<1|3|4>
    LPGR_BAYER8_W, LPGR_BAYER8_P, LPGR_BAYER16_W, LPGR_BAYER16_P              // mosaics: bayer_kernel4<uint8_t>, bayer_kernel<uint8_t>, ...<uint16_t>
};
enum LpClaheLut { LPCL_NONE, LPCL_COL16_256X8, LPCL_COL16_1024, LPCL_WAVE32 };   // equaliser off; clahe_lut_kernel2<256, 8>, clahe_lut_kernel2<1024>, clahe_lut_kernel
enum LpClaheInterp { LPCI_NONE, LPCI_PX4, LPCI_PX1 };                            // equaliser off; clahe_interp_kernel4, clahe_interp_kernel
enum LpPyramid { LPP_COPY, LPP_OWN };     // pyramid_kernel copies the image into level 0 | level 0 IS the handle's equalised image: no copy
enum LpDetFirst { LPDF_NONE, LPDF_TILE, LPDF_STRIP };   // caller-side corner list: no detector; mineig_nms_kernel, mineig_nms_strip_kernel
enum LpSubpix { LPSP_NONE, LPSP_WIDE_WIN, LPSP_GENERIC, LPSP_X16, LPSP_STOCK };   // subpix_wide_kernel, subpix_generic_kernel, subpix_kernel16, subpix_kernel
enum LpKlt { LPKL_K3, LPKL_K16 };         // klt_kernel3, klt_kernel16
enum LpAnnounce { LPA_NONE, LPA_SIGNAL, LPA_EVENT };   // how "the corners of this frame are there" reaches book-keeping's refill half
enum LpBook {
    LPB_PLAIN,       // ransac_kernel, bookkeep_a_kernel, bookkeep_b_kernel on one stream: the caller's corner list (and the direct-track entry point)
    LPB_JOIN,        // the same kernels, RANSAC on the side stream, which joins back in front of book-keeping: the device detector outside run-ahead mode
    LPB_FUSED,       // ransac_book_kernel: RANSAC and both halves of book-keeping in ONE launch on the side stream
    LPB_PAIR         // ransac_book_a_kernel, bookkeep_b_kernel on the side stream
};

// what a call is made with.  Of the handle: the first three blocks; of the call: the fourth; of the process / the handle's queues: the last
struct FrontIn {
    int batch = 1;
    bool throughput = false;       // the throughput forms of the image kernels (rvio_hip::wide_px: batch handles of >= 8 instances; rvio_hip_debug_kernel_forms)
    int W = 0, H = 0, F = 0, nmax = 0;
    bool equalizer = false;
    int cl_tx = 0, cl_ty = 0, cl_tw = 0, cl_th = 0;   // CLAHE tile grid and tile size
    int sp_win = LP_SP_WIN;        // cornerSubPix half-window, floor(Tracker.nMinDist / 2)
    int channels = 1;              // samples per pixel of the caller's images (1: mono or a mosaic)

    bool piped_call = false;       // a whole-frame call of the pipelined path (else: a per-stage entry point, everything on the filter stream)
    bool have_corner_list = false; // the caller hands in the corners: no device detector
    long frame_no = 0;
    bool first_cleared = false;    // mbIsTheFirstImage has gone to 0 in every instance (it never comes back: Tracker.cc:233)
    bool src_dword = false;        // the caller's image: base address, row stride and instance stride are multiples of four bytes

    bool no_runahead = false;      // RVIO_NO_RUNAHEAD
    bool no_device_polls = false;  // RVIO_PARANOID's bit 4, or a counter-collecting profiler that serialises kernels across queues
    bool own_queues = false;       // the handle's four streams own their hardware queues and nothing else feeds queues beside them:
                                   // private_queues && !queues_shared && !extra_queues
    // raw sensor data (rvio_hip_set_image_format): both off = the 8-bit formats above
    int bits = 8;                  // bits per sample: 8 | 16
    bool bayer = false;            // the image is a Bayer mosaic (channels == 1): converted even at one byte per pixel
};

struct FrontForms {
    // ---- mode
    bool use_det = false;        // FeatureDetector::DetectWithSubPix on the device
    bool piped = false;
    bool runahead = false;       // pipelined whole-frame call with the device detector: image chains of consecutive frames in flight, book-keeping on the side stream
    bool dev_sync = false;       // ... of ONE instance: hand-over -> filter and corners -> refill go through device-side counters (StageSync)
    int par = 0;                 // frame parity of a piped call, else 0
    int dslot = 0;               // corner list / count of this call: three in rotation in run-ahead mode, else by parity
    int ic = 0;                  // image chain of a run-ahead call: its stream, event and counters (< plan.n_ic); else 0
    int lut_set = 0;             // CLAHE LUT set
    int det_set = 0;             // detector scratch set
    // ---- synchronisation
    bool filter_done_by_counter = false;   // "the filter of this frame has finished" is stage_sync->aug reaching a target (no marker packet on the filter stream), else an event
    bool wait_book_k3 = false;             // the image chain starts behind book-keeping(k-3): it rewrites equalised image k % 4 and corner list k % 3
    bool wait_first_flag = false;          // the detector's threshold pass waits for book-keeping(k-1): it reads mbIsTheFirstImage
    bool pyr_on_image = false;             // the pyramid rides on the image chain (run-ahead mode with the equaliser): the side stream's KLT has to be told when it is there
    bool klt_polls_pyramid = false;        // ... klt_kernel3 polls the image chain's pyramid counter itself; else an event (evC) in front of it on the side stream
    bool det_folds_signal = false;         // ... which the detector's first launch bumps, right behind the pyramid on the chain's queue (the tile form: the strip
                                           // form has no folded signal, and the poll is never taken with it)
    bool fork_side = false;                // the side stream forks from the image stream with an event of its own (evD0): nothing above has ordered it yet
    LpAnnounce corners = LPA_NONE;
    // ---- stream roles
    LpStream base = LPR_FILTER;   // the call's own stream: where everything runs that is not forked off
    LpStream image = LPR_FILTER;  // gray, CLAHE, detector
    LpStream pyr = LPR_FILTER;    // the pyramid
    LpStream side = LPR_FILTER;   // KLT, RANSAC
    LpStream book = LPR_FILTER;   // book-keeping: the hand-over event is recorded here
    // ---- kernel forms
    LpGray gray = LPGR_NONE;             LpLaunch gray_l;
    LpClaheLut clahe_lut = LPCL_NONE;    LpLaunch clahe_lut_l;
    LpClaheInterp clahe_interp = LPCI_NONE; LpLaunch clahe_interp_l;
    LpPyramid pyramid = LPP_COPY;        LpLaunch pyramid_l;
    LpDetFirst det_first = LPDF_NONE;    LpLaunch det_first_l;
    LpLaunch neigh_l, greedy_l;
    LpSubpix subpix = LPSP_NONE;         LpLaunch subpix_l;
    LpKlt klt = LPKL_K3;                 LpLaunch klt_l;
    LpBook book_form = LPB_PLAIN;
    LpLaunch ransac_l;                   // the launch RANSAC is in: ransac_kernel, ransac_book_a_kernel or ransac_book_kernel
    LpLaunch book_a_l, book_b_l;         // bookkeep_a_kernel, bookkeep_b_kernel where they are launches of their own
};

inline FrontForms front_forms(const LaunchPlan& p, const FrontIn& in) {
    FrontForms f;
    const int B = in.batch, W = in.W, H = in.H, F = in.F;
    const bool wide = in.throughput;
    // ---- mode.  Two of them:
    //  * plain (per-stage calls, or a caller-side corner list): one image stream; the side stream joins back and book-keeping runs on the call's stream;
    //  * run-ahead (pipelined whole-frame path with the device detector): book-keeping runs on the SIDE stream, so the image stream is free for CLAHE +
    //    detector of frame k+1 as soon as the detector of frame k is done — the image chain never reads tracker state, except mbIsTheFirstImage (the
    //    detector's distance factor), hence one wait on book-keeping(k-1) in front of the threshold pass.  What book-keeping(k) still reads while frame
    //    k+1 is being detected is buffered in rotation (equalised image, corner list).
    f.use_det = !in.have_corner_list;   // no corner list from the caller: run FeatureDetector::DetectWithSubPix on the device
    f.piped = in.piped_call;
    f.par = f.piped ? (int)(in.frame_no & 1) : 0;
    f.runahead = f.piped && f.use_det && !in.no_runahead;
    // device-side counters for ONE instance only: a batch handle's kernels have one workgroup per instance, and a counter says nothing about which of them have finished
    f.dev_sync = f.runahead && B == 1 && !in.no_device_polls;
    f.dslot = f.runahead ? (int)(in.frame_no % 3) : f.par;
    // in run-ahead mode the image chains of consecutive frames alternate between plan.n_ic streams (each with its own detector scratch and CLAHE LUTs), so
    // that as many are in flight — the chain is ~150 us long, the longest of the frame, and with one stream it WAS the frame period
    // (outside run-ahead mode there is ONE image stream, the call's own: no chain to name; the LUTs still alternate by parity)
    f.ic = f.runahead ? (int)(in.frame_no % p.n_ic) : 0;
    f.lut_set = f.runahead ? f.ic : f.par;
    f.det_set = f.runahead ? f.ic : 0;
    // ---- synchronisation
    // single instance in run-ahead mode: the filter's last kernel bumps the device-side counter (book-keeping of a later frame polls it); otherwise an event behind it
    f.filter_done_by_counter = f.dev_sync;
    // Run-ahead mode: the image chain of frame k (CLAHE, detector; with the equaliser also the pyramid) rewrites buffers that book-keeping / KLT of earlier
    // frames read — equalised image k % 4, corner list and count k % 3 — so it starts behind book-keeping(k-3), with or without the equaliser (the detector
    // alone rewrites det_xy2[k % 3] / det_nout[k % 3], which bookkeep_b(k-3) reads).
    f.wait_book_k3 = f.runahead && in.frame_no >= 3;
    // run-ahead: book-keeping(k-1) ran on the side stream; its event also says that mbIsTheFirstImage is final ... until the flag has gone to 0 in every
    // instance: the host sees that in the mirror book-keeping writes (a stale 1 only keeps the wait one frame longer) and the detector chain then paces itself
    f.wait_first_flag = f.runahead && in.frame_no >= 1 && !in.first_cleared;
    // With the equaliser the pyramid of a run-ahead frame rides on the image chain (see the stream roles), and the side stream's KLT has to wait for it.  klt_kernel3 polls
    // the chain's counter itself (no barrier packet on the side stream) —
    //  * own_queues: on a handle whose four streams own their hardware queues only (the first live handle of the process): 200 polling workgroups per frame
    //    in front of kernels of OTHER handles on a shared queue timed the eight-handle leg of the bench out (a consumer may only spin where everything it
    //    waits for was submitted earlier to queues nobody else feeds) ... and not on a handle that runs the sharded frame over a real collective,
    //  * 6 nmax <= 96: nor at long windows (the Cholesky factor's launches share the copy queue): with the forced-sharded cfg E run of the bench two runs in
    //    six stalled for the poll's full 30 s (none in six without it) — more busy queues than the command processor keeps resident, and a queue of spinning
    //    workgroups in front of the one that would release them,
    //  * !throughput: klt_kernel16 has no poll, and the strip form of the detector's first pass no folded signal.
    // Without it: an event (evC) recorded behind the pyramid, which the side stream waits for.
    f.pyr_on_image = in.equalizer && f.runahead;
    f.klt_polls_pyramid = f.pyr_on_image && f.dev_sync && in.own_queues && 6 * in.nmax <= 96 && !wide;
    f.fork_side = f.use_det && !f.pyr_on_image;   // (there the pyramid's event or counter has ordered the side stream behind the image already)
    // corners of frame k ready (the refill half of book-keeping on the side stream waits for it): a one-workgroup signal behind cornerSubPix that
    // book-keeping polls, or a stream-level event.  (One counter per image chain: each has ONE producer queue, so "count >= the frames this chain has been
    // handed" means THIS frame's corners.)
    f.corners = !f.use_det ? LPA_NONE : f.dev_sync ? LPA_SIGNAL : f.runahead ? LPA_EVENT : LPA_NONE;
    // ---- stream roles.  The IMAGE stream carries CLAHE and FeatureDetector::DetectWithSubPix: the longest chain, ~170 us; the side stream pyramid, KLT,
    // RANSAC: ~90 us
    f.base = f.piped ? LPR_TRACKER : LPR_FILTER;
    f.image = f.runahead ? LPR_IMAGE : f.base;
    f.side = f.use_det ? LPR_SIDE : f.base;      // fork: pyramid / KLT / RANSAC go to the side stream, the detector stays where the image was completed
    // the pyramid of an equalised run-ahead frame rides on the image stream: it needs nothing from the side stream's chain (KLT(k-1), RANSAC, book-keeping),
    // which is the longest serial chain of the front end — 19 us less of it; the image chain has the slack
    f.pyr = f.pyr_on_image ? f.image : f.side;
    f.book = f.runahead ? LPR_SIDE : f.base;
    // ---- kernel forms
    // gray conversion: B interleaved images -> B packed gray images.  The dword form wherever every row of every instance starts on a dword and holds whole
    // groups of four pixels, the byte form otherwise (same bits: gray.h)
    // Raw sensor data (raw.hip) has the same two forms under the same condition: 16-bit samples put a lane's four pixels into 2 / 6 / 8 aligned dwords,
    // a mosaic into one (8 bit) or two (16 bit) per row of its 3 x 3 window.  A mosaic of one byte per pixel is converted too: whether a conversion is
    // launched follows from the format, not from the bytes per pixel.
    const bool gray_dword = W % 4 == 0 && in.src_dword;
    const bool converted = in.channels > 1 || in.bits == 16 || in.bayer;
    if (in.bayer) f.gray = in.bits == 16 ? (gray_dword ? LPGR_BAYER16_W : LPGR_BAYER16_P) : (gray_dword ? LPGR_BAYER8_W : LPGR_BAYER8_P);
    else if (in.bits == 16) f.gray = in.channels == 1 ? (gray_dword ? LPGR_W16_1 : LPGR_P16_1) : in.channels == 3 ? (gray_dword ? LPGR_W16_3 : LPGR_P16_3)
                                                                                                                    : (gray_dword ? LPGR_W16_4 : LPGR_P16_4);
    else if (in.channels > 1) f.gray = in.channels == 3 ? (gray_dword ? LPGR_DWORD3 : LPGR_BYTE3) : (gray_dword ? LPGR_DWORD4 : LPGR_BYTE4);
    if (converted) f.gray_l = {(W + 255) / 256, (H + 3) / 4, B, 256};
    // what CLAHE reads: the caller's image, or the handle's gray buffer (row stride W, instance stride W H, slots W H B apart in one allocation)
    const bool eq_src_dword = converted ? W % 4 == 0 : in.src_dword;
    if (in.equalizer) {
        // lane-private 16-bit histogram columns, no LDS-atomic conflicts: every handle.  A counter sees the pixels of ONE lane column of the tile,
        // ceil(tw / 64) th of them — 1296 at 1080p —, so 16 bits hold for any image a camera delivers; the 32-bit per-wave form stays as the fall-back
        if (((in.cl_tw + 63) / 64) * in.cl_th <= 65535) {
            // (throughput: eight rows of byte loads in flight per thread instead of four: the histogram of a batch is load-latency bound; 135.5 -> 136.7 k frames/s at 128 streams)
            f.clahe_lut = wide ? LPCL_COL16_256X8 : LPCL_COL16_1024;
            f.clahe_lut_l = {in.cl_tx * in.cl_ty, 1, B, wide ? 256 : 1024};
        } else {
            f.clahe_lut = LPCL_WAVE32;
            f.clahe_lut_l = {in.cl_tx * in.cl_ty, 1, B, LP_CLAHE_LUT_T};
        }
        // interpolation: four pixels per thread in the throughput form where rows start on dwords and hold whole groups of four, else one
        if (wide && W % 4 == 0 && eq_src_dword) { f.clahe_interp = LPCI_PX4; f.clahe_interp_l = {(W / 4 + 63) / 64, (H + 15) / 16, B, 256}; }
        else { f.clahe_interp = LPCI_PX1; f.clahe_interp_l = {(W + 63) / 64, (H + 3) / 4, B, 256}; }
    }
    {   // the whole pyramid in one launch (pyrDown chain + the copy of the frame into level 0); one workgroup per 8x8 tile of level 3
        const int w3 = (((W + 1) / 2 + 1) / 2 + 1) / 2, h3 = (((H + 1) / 2 + 1) / 2 + 1) / 2;
        f.pyramid = in.equalizer ? LPP_OWN : LPP_COPY;   // the equalised image of frame k doubles as level 0 of frame k's pyramid
        f.pyramid_l = {(w3 + 7) / 8, (h3 + 7) / 8, B, LP_PYR_T};
    }
    if (f.use_det) {
        if (wide) {   // batch handles of >= 8 instances: the fused pass in its throughput form (one wave per strip, rows walked with the state in registers), which has no folded signal
            f.det_first = LPDF_STRIP;
            f.det_first_l = {(W + LP_DET_SW - 1) / LP_DET_SW, (H + LP_DET_SH - 1) / LP_DET_SH, B, 64};
        } else {      // one stream: min-eigenvalue map + strict 3x3 local maxima in one pass (the map stays in LDS), then the image-wide threshold on the provisional list
            f.det_first = LPDF_TILE;
            f.det_first_l = {(W + LP_DET_TW - 1) / LP_DET_TW, (H + LP_DET_FH - 1) / LP_DET_FH, B, LP_DET_T};
            f.det_folds_signal = f.klt_polls_pyramid;
        }
        // every workgroup rebuilds the candidate buckets in its LDS before it walks its share of the candidates: 8 of them for the latency of one stream,
        // fewer for batch handles, whose width comes from the streams (measured at 128 streams: 8 -> 134.5 k frames/s, 4 -> 135.3, 2 -> 136.0, 1 -> 135.9)
        f.neigh_l = {wide ? LP_NEIGH_BLOCKS_WIDE : LP_NEIGH_BLOCKS, 1, B, LP_NEIGH_T, LP_NEIGH_LDS, LPF_NEIGH};
        f.greedy_l = {1, 1, B, LP_GREEDY_T, LP_GREEDY_LDS, LPF_GREEDY};
        // cornerSubPix on the detector's raw corners
        if (in.sp_win > 15) {               // Tracker.nMinDist >= 32: the summation grid no longer fits LDS whole
            f.subpix = LPSP_WIDE_WIN; f.subpix_l = {F, 1, B, LP_SPG_T, lp_subpix_wide_lds(in.sp_win), LPF_SUBPIX_WIDE};
        } else if (in.sp_win != LP_SP_WIN) {   // a cornerSubPix window other than the stock 7: the plain form
            f.subpix = LPSP_GENERIC; f.subpix_l = {F, 1, B, LP_SPG_T};
        } else if (wide) {                  // four corners per wave
            f.subpix = LPSP_X16; f.subpix_l = {(F + 3) / 4, 1, B, 64};
        } else {
            f.subpix = LPSP_STOCK; f.subpix_l = {F, 1, B, LP_SP_T};
        }
    }
    // KLT: a wave per feature, or (batch handles of >= 8 instances) the throughput form, four features per wave
    if (wide) { f.klt = LPKL_K16; f.klt_l = {(F + 3) / 4, 1, B, 64}; }
    else { f.klt = LPKL_K3; f.klt_l = {F, 1, B, 64}; }
    // RANSAC and book-keeping.  The refill half's geometry is the plan's (book_waves waves, book_lds bytes).  A caller-side corner list is ONE list: the
    // entry points that take one address a single instance, and book-keeping of that shape is one workgroup on instance 0 whatever the batch
    const LpLaunch ransac = {1, 1, B, 256, (size_t)8 * F + 16, LPF_DEFAULT};
    const LpLaunch book_b = {1, 1, B, 64 * p.book_waves, p.book_lds, LPK_BOOKKEEP_B};
    if (!f.runahead) {
        // the side stream (long finished when the detector is) joins back in front of book-keeping; with a caller-side list there is nothing to join
        f.book_form = f.use_det ? LPB_JOIN : LPB_PLAIN;
        const int bz = f.use_det ? B : 1;
        f.ransac_l = ransac; f.book_a_l = {1, 1, bz, 256}; f.book_b_l = {1, 1, bz, book_b.threads, book_b.lds, book_b.kernel};
    } else if (f.dev_sync && p.book_fused) {
        // one instance, device-side counters: RANSAC and both halves of book-keeping are ONE launch (the refill half polls the detector's counter inside it)
        f.book_form = LPB_FUSED;
        f.ransac_l = {1, 1, B, 64 * p.book_waves, p.book_lds, LPK_RANSAC_BOOK};
    } else {
        // RANSAC rides in the launch of book-keeping's hand-over half (both one workgroup, back to back on the side stream); the refill half follows once the
        // corners are there (a poll inside it, or an event in front of it)
        f.book_form = LPB_PAIR;
        f.ransac_l = ransac; f.book_b_l = book_b;
    }
    return f;
}
