// Host build of csrc/launch_plan.h for tests/test_map_plan.py: the launch form of the map-landmark rows (map_launch), the sizes of the block the
// map calls allocate and what the plan does with the kernel's static LDS, as plain C functions.
#include <cstring>
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
long mpp_lds_limit() { return RVIO_LDS_LIMIT; }
int mpp_threads() { return LP_MAP_T; }
int mpp_waves() { return LP_MAP_WAVES; }
int mpp_points() { return LP_MAP_POINTS; }
int mpp_rows() { return LP_MAP_ROWS; }
int mpp_nmax() { return LP_FIXP_NMAX; }
int mpp_nz() { return LP_MAP_NZ; }
int mpp_aux_rows() { return LP_AUX_MAX_ROWS; }
long mpp_lds_doubles() { return LP_MAP_LDS_DOUBLES; }
double mpp_min_depth() { return LP_MAP_MIN_DEPTH; }
long mpp_H_stride(int dmax) { return (long)map_H_stride(dmax); }
long mpp_block_bytes(int batch, int dmax) { return (long)map_block_bytes(batch, dmax); }
int mpp_num_kernels() { return LPK_COUNT; }
const char* mpp_kernel_name(int k) { return (k >= 0 && k < LPK_COUNT) ? kLpKernelName[k] : ""; }
// out: gx, gy, gz, threads, dynamic LDS bytes, LpKernel
void mpp_launch(int batch, long* out) {
    const LpLaunch l = map_launch(batch);
    out[0] = l.gx; out[1] = l.gy; out[2] = l.gz; out[3] = l.threads; out[4] = (long)l.lds; out[5] = l.kernel;
}
// the plan of a handle: its refusal code, and the dynamic-LDS limit create sets for LpKernel k
int mpp_plan(int max_len, int n_features, int batch, const size_t* statics, int k, long* attr) {
    const LaunchPlan p = launch_plan(max_len, n_features, batch, statics);
    *attr = (long)p.attr[k];
    return p.rc;
}
}
