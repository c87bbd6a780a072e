// Host build of csrc/launch_plan.h for tests/test_window_plan.py: the launch form of the window-pose kernel (window_pose_launch), what the plan
// counts of its static LDS and what the plan does with the kernel's static LDS, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long wpp_lds_limit() { return RVIO_LDS_LIMIT; }
int wpp_threads() { return LP_WINP_T; }
int wpp_nmax() { return LP_FIXP_NMAX; }
int wpp_nz() { return LP_WINP_NZ; }
int wpp_groups() { return LP_WINP_GROUPS; }
int wpp_words() { return LP_WINP_WORDS; }
long wpp_chain_doubles() { return LP_FIXP_CHAIN; }
long wpp_lds_doubles() { return LP_WINP_LDS_DOUBLES; }
int wpp_num_kernels() { return LPK_COUNT; }
int wpp_kernel_id() { return LPK_WINDOW_POSE; }
const char* wpp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void wpp_launch(int batch, int n_ages, long* out) {
    const LpLaunch l = window_pose_launch(batch, n_ages);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the plan of a handle: its refusal code, and the dynamic-LDS limit create sets for LpKernel k
int wpp_plan(int max_len, int n_features, int batch, const size_t* statics, int k, long* attr) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    *attr = (long)p.attr[k];
    return p.rc;
}
}
