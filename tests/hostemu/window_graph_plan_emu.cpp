// Host build of csrc/launch_plan.h for tests/test_window_graph_plan.py: the launch forms of the window-edge and window-joint kernels
// (window_edge_launch, window_joint_launch), what the plan counts of their static LDS and what the plan does with it, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long wgp_lds_limit() { return RVIO_LDS_LIMIT; }
int wgp_nmax() { return LP_FIXP_NMAX; }
int wgp_max_len() { return RVIO_MAX_LEN; }
long wgp_chain_doubles() { return LP_FIXP_CHAIN; }
int wgp_edge_threads() { return LP_WEDGE_T; }
int wgp_edge_nz() { return LP_WEDGE_NZ; }
int wgp_edge_groups() { return LP_WEDGE_GROUPS; }
int wgp_edge_words() { return LP_WEDGE_WORDS; }
int wgp_edge_max_pairs() { return LP_WEDGE_MAX_PAIRS; }
long wgp_edge_lds_doubles() { return LP_WEDGE_LDS_DOUBLES; }
int wgp_joint_threads() { return LP_WJNT_T; }
long wgp_joint_lds_doubles() { return LP_WJNT_LDS_DOUBLES; }
long wgp_pose_lds_doubles() { return LP_WINP_LDS_DOUBLES; }
int wgp_pose_nz() { return LP_WINP_NZ; }
int wgp_pose_groups() { return LP_WINP_GROUPS; }
int wgp_num_kernels() { return LPK_COUNT; }
int wgp_edge_id() { return LPK_WINDOW_EDGE; }
int wgp_joint_id() { return LPK_WINDOW_JOINT; }
const char* wgp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void wgp_edge_launch(int batch, int n_pairs, long* out) {
    const LpLaunch l = window_edge_launch(batch, n_pairs);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
void wgp_joint_launch(int batch, int n_ages, long* out) {
    const LpLaunch l = window_joint_launch(batch, n_ages);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the plan of a handle: its refusal code, and the dynamic-LDS limit create sets for LpKernel k
int wgp_plan(int max_len, int n_features, int batch, const size_t* statics, int k, long* attr) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    *attr = (long)p.attr[k];
    return p.rc;
}
}
