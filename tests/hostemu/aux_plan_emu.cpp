// Host build of csrc/launch_plan.h for tests/test_aux_plan.py: the launch form of the auxiliary measurement update (aux_update_launch) and the
// limit the plan sets for its two kernel instances, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long ap_lds_limit() { return RVIO_LDS_LIMIT; }
int ap_max_rows() { return LP_AUX_MAX_ROWS; }
int ap_threads() { return LP_AUX_T; }
const char* ap_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void ap_launch(int n, int m, int batch, long* out) {
    const LpLaunch l = aux_update_launch(n, m, batch);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the dynamic-LDS limit create sets for LpKernel k on a handle of max_len; -1: the configuration is refused
long ap_attr(int max_len, int n_features, int batch, const size_t* statics, int k) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    return p.rc ? -1 : (long)p.attr[k];
}
int ap_num_kernels() { return LPK_COUNT; }
int ap_splits(int G) { return aux_splits(G); }
}
