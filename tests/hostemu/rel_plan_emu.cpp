// Host build of csrc/launch_plan.h for tests/test_rel_plan.py: the launch form of the relative-pose rows (rel_launch) and what the plan does with
// the kernel's static LDS, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long rlp_lds_limit() { return RVIO_LDS_LIMIT; }
int rlp_threads() { return LP_FIXP_T; }
int rlp_nmax() { return LP_FIXP_NMAX; }
int rlp_chain_doubles() { return LP_FIXP_CHAIN; }
int rlp_num_kernels() { return LPK_COUNT; }
const char* rlp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void rlp_launch(int batch, long* out) {
    const LpLaunch l = rel_launch(batch);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the plan of a handle: its refusal code, and the dynamic-LDS limit create sets for LpKernel k
int rlp_plan(int max_len, int n_features, int batch, const size_t* statics, int k, long* attr) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    *attr = (long)p.attr[k];
    return p.rc;
}
}
