// The rvio_fix records the host hands to the library, without a device: this program links host/rvio_host.cpp and defines the four library
// entry points that path uses itself (a definition in the program wins over the shared library's), so every record that reaches
// rvio_hip_update_fix / rvio_hip_update_fix_past is printed instead of fused.  tests/test_fix_host.py compares the bytes.
//   argv[1]: a fix file (parse_fixes).  Output, one line per record, `<tag> <kind> <256 hex digits>`:
//     builder       the free builders position_fix / attitude_fix / pose_fix / gravity_fix on the values below
//     typed         System::fix_position / _attitude / _pose / _gravity on the same values
//     typed_past    System::fix_*_at on the same values, at a stamp inside the window
//     queued        System::apply_fixes on the parsed file, no latency (every row through rvio_hip_update_fix)
//     queued_past   System::apply_fixes on the parsed file with latency 0 and a window that holds every stamp (GRAVITY: still `queued`)
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#define private public   // System::ready_, stamps_, apply_fixes: reached here only, the class is laid out the same
#include "rvio_host.hpp"
#undef private

static const char* g_tag = "";
static void print_record(const char* suffix, int kind, const rvio_fix* f) {
    unsigned char b[sizeof *f];
    std::memcpy(b, f, sizeof b);
    std::printf("%s%s %d ", g_tag, suffix, kind);
    for (unsigned char c : b) std::printf("%02x", c);
    std::printf("\n");
}
static int g_dummy;
extern "C" {
int rvio_hip_create(const rvio_config*, int, rvio_hip** out) { *out = (rvio_hip*)&g_dummy; return RVIO_OK; }
void rvio_hip_destroy(rvio_hip*) {}
int rvio_hip_update_fix(rvio_hip*, int, int kind, int, const rvio_fix* fix) { print_record("", kind, fix); return RVIO_OK; }
int rvio_hip_update_fix_past(rvio_hip*, int, int kind, int, int, double, const rvio_fix* fix) { print_record("_past", kind, fix); return RVIO_OK; }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const double p[3] = {1.0, -2.0, 3.5}, q[4] = {0.0, 0.6, 0.0, 0.8}, sp[3] = {0.1, 0.2, 0.3}, sq[3] = {0.01, 0.02, 0.03}, lever[3] = {0.3, -0.2, 0.1};
    const double a[3] = {0.0, 9.8, 0.1};
    g_tag = "builder";
    const rvio_fix b0 = rvio::position_fix(p, sp, lever), b0n = rvio::position_fix(p, sp, nullptr), b1 = rvio::attitude_fix(q, sq);
    const rvio_fix b2 = rvio::pose_fix(p, q, sp, sq, lever), b3 = rvio::gravity_fix(a, sp);
    print_record("", RVIO_FIX_POSITION, &b0); print_record("", RVIO_FIX_POSITION, &b0n); print_record("", RVIO_FIX_ATTITUDE, &b1);
    print_record("", RVIO_FIX_POSE, &b2); print_record("", RVIO_FIX_GRAVITY, &b3);

    std::vector<rvio::FixRow> rows;
    std::string err;
    if (!rvio::read_fixes(argv[1], &rows, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    rvio::Settings s{};
    rvio::System sys(s, 0);
    if (!sys.ok()) return 3;
    sys.ready_ = true;
    g_tag = "typed";
    if (sys.fix_position(p, sp, lever, false) || sys.fix_position(p, sp, nullptr, false) || sys.fix_attitude(q, sq, false) || sys.fix_pose(p, q, sp, sq, lever, false) ||
        sys.fix_gravity(a, sp, false)) return 4;
    sys.stamps_ = {1000.0, 999.0, -1000.0};   // newest first: every stamp of the file lies in the window
    if (sys.fix_position_at(999.5, p, sp, lever, false) || sys.fix_position_at(999.5, p, sp, nullptr, false) || sys.fix_attitude_at(999.5, q, sq, false) ||
        sys.fix_pose_at(999.5, p, q, sp, sq, lever, false)) return 4;
    g_tag = "queued";
    sys.queue_fixes(rows, false);
    if (sys.apply_fixes(1e9) < 0 || sys.fixes_applied() != (long)rows.size()) return 5;
    sys.queue_fixes(rows, false, 0.0);
    if (sys.apply_fixes(1e9) < 0 || sys.fixes_applied() != (long)rows.size() || sys.fixes_dropped() != 0) return 5;
    // a kind the parser never produces: refused by name, nothing handed on
    rows.assign(1, rvio::FixRow());
    rows[0].kind = 7;
    sys.queue_fixes(rows, false);
    g_tag = "unknown";
    if (sys.apply_fixes(1e9) >= 0 || sys.error() != "System: a queued fix of unknown kind") return 6;
    sys.h_ = nullptr;
    return 0;
}
