// plan_emu.cpp — r-vio_amd/csrc/launch_plan.h compiled with g++: the launch geometry create_impl derives from a configuration, evaluated on the
// CPU for every accepted (max_track_len, n_features, batch), the forms of an update (update_forms) for every clone count of every window, and the
// forms of a front-end call (front_forms) for every mode, geometry and environment a call can be made in.
// tests/test_launch_plan.py feeds it the static LDS of each kernel as the built library's code object has it and checks static + dynamic against a CU's LDS.
#include "../../r-vio_amd/csrc/launch_plan.h"
#include <initializer_list>
#include <string.h>

extern "C" {
int lp_num_kernels() { return LPK_COUNT; }
const char* lp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
long lp_lds_limit() { return RVIO_LDS_LIMIT; }
int lp_max_features() { return RVIO_MAX_FEATURES; }
int lp_max_len() { return RVIO_MAX_LEN; }

// one configuration.  attr[LPK_COUNT]: dynamic LDS per kernel; info[18]: see below; why: the refusal's text (<= 255 chars).  Returns plan.rc
int lp_eval(int max_len, int n_features, int batch, const size_t* statics, size_t* attr, long* info, char* why) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    for (int k = 0; k < LPK_COUNT; ++k) attr[k] = p.attr[k];
    info[0] = p.book_waves; info[1] = (long)p.book_lds; info[2] = p.book_fused; info[3] = p.tm_global; info[4] = p.lit_state_global;
    info[5] = p.solve5_variant; info[6] = p.solve7_variant; info[7] = p.solve9_nt; info[8] = p.n_ic; info[9] = p.feat_threads;
    info[10] = (long)p.feat_lds; info[11] = (long)p.fprop_lds; info[12] = (long)p.trunc_lds; info[13] = p.fuse_ok; info[14] = (long)p.jb_lds; info[15] = (long)p.gram_batch_lds;
    info[16] = p.chol_queue; info[17] = p.lit_ok;
    why[0] = 0;
    if (p.why) { strncpy(why, p.why, 255); why[255] = 0; }
    return p.rc;
}

// every max_track_len in [ml0, ml1] x every n_features in [f0, f1] at one batch size.  worst[k]: the largest static + dynamic of kernel k over the
// supported configurations, at worst_cfg[2k] = max_len, worst_cfg[2k + 1] = n_features.  first_bad[3]: {kernel, max_len, n_features} of the first
// supported configuration with a kernel over the limit.  Returns the number of such (configuration, kernel) pairs; *n_unsupported: refused configurations.
long lp_sweep(int ml0, int ml1, int f0, int f1, int batch, const size_t* statics, size_t* worst, int* worst_cfg, int* first_bad, long* n_unsupported) {
    long bad = 0, uns = 0;
    for (int k = 0; k < LPK_COUNT; ++k) { worst[k] = 0; worst_cfg[2 * k] = worst_cfg[2 * k + 1] = 0; }
    for (int ml = ml0; ml <= ml1; ++ml)
        for (int F = f0; F <= f1; ++F) {
            const LaunchPlan p = launch_plan(ml, F, batch, statics);
            if (p.rc) { ++uns; continue; }
            for (int k = 0; k < LPK_COUNT; ++k) {
                if (!p.attr[k]) continue;
                const size_t tot = p.attr[k] + statics[k];
                if (tot > worst[k]) { worst[k] = tot; worst_cfg[2 * k] = ml; worst_cfg[2 * k + 1] = F; }
                if (tot > RVIO_LDS_LIMIT) { if (!bad) { first_bad[0] = k; first_bad[1] = ml; first_bad[2] = F; } ++bad; }
            }
        }
    *n_unsupported = uns;
    return bad;
}

// the forms of one update of that configuration at clone count n (update_forms).  out[LP_FORMS_LEN]: the enums and grids in the order below, then
// (bytes, LpKernel) of each launch with dynamic LDS — reduction, literal sweep, T product, solve, first Joseph launch, final_lds_kernel.  Returns plan.rc
enum { LP_FORMS_LEN = 32 };
int lp_forms_len() { return LP_FORMS_LEN; }
int lp_forms(int max_len, int n_features, int batch, const size_t* statics, int n, int pre, int whole_update, int combined, int lit, long* out) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    if (p.rc) return p.rc;
    const UpdateForms f = update_forms(p, batch, n, pre != 0, whole_update != 0, combined != 0, lit != 0);
    int k = 0;
    out[k++] = f.chol; out[k++] = f.gram; out[k++] = f.gram_grid; out[k++] = f.gram_finish; out[k++] = f.lit_batch;
    out[k++] = f.tprod; out[k++] = f.tprod_grid; out[k++] = f.solve; out[k++] = f.split_nt; out[k++] = f.own_chol; out[k++] = f.dx;
    out[k++] = f.joseph; for (int g = 0; g < 4; ++g) out[k++] = f.grid[g];
    out[k++] = f.role_wgs;
    for (const LpLds* l : {&f.gram_lds, &f.lit_lds, &f.tprod_lds, &f.solve_lds, &f.ug_lds, &f.fin_lds}) { out[k++] = (long)l->bytes; out[k++] = l->kernel; }
    while (k < LP_FORMS_LEN) out[k++] = 0;
    return 0;
}

// the forms of one front-end call of that configuration (front_forms).  in[LP_FRONT_IN]: the fields of FrontIn in the order below.  out[LP_FRONT_LEN]:
// mode, synchronisation flags, stream roles, form enums, then (gx, gy, gz, threads, lds, kernel) of each launch in the order of FrontForms.  Returns plan.rc
enum { LP_FRONT_IN = 18, LP_FRONT_LEN = 120 };
int lp_front_in_len() { return LP_FRONT_IN; }
int lp_front_len() { return LP_FRONT_LEN; }
long lp_subpix_wide_lds_bytes(int win) { return (long)lp_subpix_wide_lds(win); }
long lp_neigh_lds() { return LP_NEIGH_LDS; }
long lp_greedy_lds() { return LP_GREEDY_LDS; }
int lp_front_forms(int max_len, int n_features, int batch, const size_t* statics, const long* in, long* out) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    if (p.rc) return p.rc;
    FrontIn i;
    int k = 0;
    i.batch = batch; i.F = n_features; i.nmax = max_len - 1;
    i.throughput = in[k++] != 0; i.W = (int)in[k++]; i.H = (int)in[k++];
    i.equalizer = in[k++] != 0; i.cl_tx = (int)in[k++]; i.cl_ty = (int)in[k++]; i.cl_tw = (int)in[k++]; i.cl_th = (int)in[k++];
    i.sp_win = (int)in[k++]; i.channels = (int)in[k++];
    i.piped_call = in[k++] != 0; i.have_corner_list = in[k++] != 0; i.frame_no = in[k++]; i.first_cleared = in[k++] != 0; i.src_dword = in[k++] != 0;
    i.no_runahead = in[k++] != 0; i.no_device_polls = in[k++] != 0; i.own_queues = in[k++] != 0;
    const FrontForms f = front_forms(p, i);
    k = 0;
    out[k++] = f.use_det; out[k++] = f.piped; out[k++] = f.runahead; out[k++] = f.dev_sync; out[k++] = f.par; out[k++] = f.dslot; out[k++] = f.ic;
    out[k++] = f.lut_set; out[k++] = f.det_set;
    out[k++] = f.filter_done_by_counter; out[k++] = f.wait_book_k3; out[k++] = f.wait_first_flag; out[k++] = f.pyr_on_image; out[k++] = f.klt_polls_pyramid;
    out[k++] = f.det_folds_signal; out[k++] = f.fork_side; out[k++] = f.corners;
    out[k++] = f.base; out[k++] = f.image; out[k++] = f.pyr; out[k++] = f.side; out[k++] = f.book;
    out[k++] = f.gray; out[k++] = f.clahe_lut; out[k++] = f.clahe_interp; out[k++] = f.pyramid; out[k++] = f.det_first; out[k++] = f.subpix; out[k++] = f.klt;
    out[k++] = f.book_form;
    for (const LpLaunch* l : {&f.gray_l, &f.clahe_lut_l, &f.clahe_interp_l, &f.pyramid_l, &f.det_first_l, &f.neigh_l, &f.greedy_l, &f.subpix_l, &f.klt_l,
                              &f.ransac_l, &f.book_a_l, &f.book_b_l}) {
        out[k++] = l->gx; out[k++] = l->gy; out[k++] = l->gz; out[k++] = l->threads; out[k++] = (long)l->lds; out[k++] = l->kernel;
    }
    while (k < LP_FRONT_LEN) out[k++] = 0;
    return 0;
}

// diagnostics in the [A|b] block: one past the last double written (stamps: the instrumented build), and the block's size
long lp_diag_end(int max_len, int stamps) { return (long)lit_diag_end(6 * (max_len - 1) + 1, stamps != 0); }
long lp_block_doubles(int max_len) { const long ldh = 6 * (max_len - 1) + 1; return 2 * ldh * ldh; }
long lp_book_lds_bytes(int F, int waves) { return (long)book_lds_bytes(F, waves); }
}
