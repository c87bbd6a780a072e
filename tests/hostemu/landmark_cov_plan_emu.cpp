// Host build of csrc/launch_plan.h for tests/test_landmark_cov_model.py: the launch form of the landmark-covariance kernel
// (landmark_cov_launch), what the plan counts of its static LDS and what the plan does with it, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
int lcp_threads() { return LP_LMC_T; }
int lcp_nmax() { return LP_FIXP_NMAX; }
int lcp_lmax() { return LP_LMC_LMAX; }
int lcp_nz() { return LP_LMC_NZ; }
int lcp_rows() { return LP_LMC_ROWS; }
int lcp_groups() { return LP_LMC_GROUPS; }
int lcp_ents() { return LP_LMC_ENTS; }
int lcp_words() { return LP_LMC_WORDS; }
double lcp_pivot_eps() { return LP_LMC_PIVOT_EPS; }
long lcp_lds_doubles() { return LP_LMC_LDS_DOUBLES; }
int lcp_num_kernels() { return LPK_COUNT; }
int lcp_kernel_id() { return LPK_LANDMARK_COV; }
const char* lcp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void lcp_launch(int batch, int slots, long* out) {
    const LpLaunch l = landmark_cov_launch(batch, slots);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the plan of a handle: its refusal code, and the dynamic-LDS limit create sets for LpKernel k
int lcp_plan(int max_len, int n_features, int batch, const size_t* statics, int k, long* attr) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    *attr = (long)p.attr[k];
    return p.rc;
}
}
