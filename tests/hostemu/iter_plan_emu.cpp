// Host build of csrc/launch_plan.h for tests/test_iter_plan.py: the launch form of one pass of the iterated measurement update
// (aux_iter_launch), the limit the plan sets for its two kernel instances and the layout of the chain's per-instance block, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long ip_lds_limit() { return RVIO_LDS_LIMIT; }
int ip_max_iters() { return LP_MEAS_MAX_ITERS; }
int ip_threads() { return LP_AUX_T; }
const char* ip_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
int ip_num_kernels() { return LPK_COUNT; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel; plain: the plain update's launch on the same window and rows
void ip_launch(int n, int m, int batch, int plain, long* out) {
    const LpLaunch l = plain ? aux_update_launch(n, m, batch) : aux_iter_launch(n, m, batch);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the dynamic-LDS limit create sets for LpKernel k on a handle of max_len; -1: the configuration is refused
long ip_attr(int max_len, int n_features, int batch, const size_t* statics, int k) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    return p.rc ? -1 : (long)p.attr[k];
}
long ip_x0_stride(int nmax) { return (long)meas_iter_x0_stride(nmax); }
long ip_block_bytes(int batch, int nmax, int dmax) { return (long)meas_iter_block_bytes(batch, nmax, dmax); }
}
