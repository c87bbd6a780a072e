// raw_plan_emu.cpp — front_forms() of r-vio_amd/csrc/launch_plan.h compiled with g++, reduced to what the image format decides: the form of the gray
// conversion with its launch, and the form of CLAHE's interpolation behind it (which reads the handle's gray buffer once anything is converted).
// tests/test_raw_plan.py sweeps it over every format.  The plan's static-LDS input plays no part in these forms: it is handed in as zeros.
#include "../../r-vio_amd/csrc/launch_plan.h"

extern "C" {
int rp_lds_limit() { return RVIO_LDS_LIMIT; }
// in: batch, throughput, W, H, equalizer, channels, bits, bayer, src_dword.  out: gray, gx, gy, gz, threads, lds, kernel, clahe_interp
int rp_front(const long* in, long* out) {
    size_t statics[LPK_COUNT] = {};
    const int batch = (int)in[0];
    const LaunchPlan p = launch_plan(11, 200, batch, statics);
    if (p.rc) return p.rc;
    FrontIn i;
    i.batch = batch; i.F = 200; i.nmax = 10;
    i.throughput = in[1] != 0; i.W = (int)in[2]; i.H = (int)in[3];
    i.equalizer = in[4] != 0; i.cl_tx = 8; i.cl_ty = 8; i.cl_tw = (i.W + 7) / 8; i.cl_th = (i.H + 7) / 8;
    i.channels = (int)in[5];
    if (in[6] != 8) i.bits = (int)in[6];          // (left alone for the 8-bit formats: the defaults must reproduce them)
    if (in[7]) i.bayer = true;
    i.src_dword = in[8] != 0;
    const FrontForms f = front_forms(p, i);
    out[0] = f.gray; out[1] = f.gray_l.gx; out[2] = f.gray_l.gy; out[3] = f.gray_l.gz; out[4] = f.gray_l.threads; out[5] = (long)f.gray_l.lds;
    out[6] = f.gray_l.kernel; out[7] = f.clahe_interp;
    return 0;
}
// the enum values by name, so that the test does not restate the header's numbering for the NEW forms
int rp_form(const char* name) {
    const struct { const char* n; int v; } t[] = {
        {"W16_1", LPGR_W16_1}, {"P16_1", LPGR_P16_1}, {"W16_3", LPGR_W16_3}, {"P16_3", LPGR_P16_3}, {"W16_4", LPGR_W16_4}, {"P16_4", LPGR_P16_4},
        {"BAYER8_W", LPGR_BAYER8_W}, {"BAYER8_P", LPGR_BAYER8_P}, {"BAYER16_W", LPGR_BAYER16_W}, {"BAYER16_P", LPGR_BAYER16_P},
        {"PX4", LPCI_PX4}, {"PX1", LPCI_PX1}, {"CI_NONE", LPCI_NONE}};
    for (const auto& e : t) { const char *a = e.n, *b = name; while (*a && *a == *b) { ++a; ++b; } if (!*a && !*b) return e.v; }
    return -1;
}
}
