// host/rvio_replay.cpp — offline replay of a EuRoC ASL folder through the MI355X hot path: the role of the reference's
// rvio_mono ROS node + rosbag play (rvio_mono.cc:54-137), without ROS.  Sensor packets are pushed in time order exactly as
// the two ROS callbacks would (every image triggers System::MonoVIO, rvio_mono.cc:78-80); poses are written in the format
// of stamped_pose_ests.dat (System.cc:369-374).
//
//   rvio_replay <settings.yaml> <asl_root> [<poses_out.dat>] [--device N] [--max-frames K] [--landmarks FILE] [--landmark-cov FILE] [--odometry FILE [--odometry-ring N]]
//                                        [--imu-odometry FILE [--imu-odometry-ring N] [--imu-odometry-cov]]
//                                        --imu-odometry: the pose and velocity behind every IMU sample the filter consumes, read in bulk from the handle's
//                                        IMU-rate ring of N samples (default 4096; System::record_imu_odometry_to); --imu-odometry-cov: every
//                                        line also carries the upper triangles of the sample's pose covariance (21) and velocity covariance (6)
//                                        --odometry: pose, velocity and pose covariance of every frame, read in bulk from the handle's ring of N
//                                        records (default 256; System::record_odometry_to); without <poses_out.dat> no frame is drained for its pose
//                                        [--smoothed FILE [--smoothed-lag L] [--smoothed-ring N]]
//                                        --smoothed: the fixed-lag smoothed trajectory — pose and pose covariance of the frame L images back (default:
//                                        max_track_len - 1, the most-smoothed pose still in the window) as the clone window holds it behind every frame,
//                                        read in bulk from the handle's smoothed ring of N records (default 256; System::record_smoothed_to); one line
//                                        per record in the layout of --odometry, stamped with the image it describes
//                                        [--edges FILE [--edges-span K] [--edges-ring N]]
//                                        --edges: a pose-graph back end's between-factors — the relative pose, with its own 6 x 6 covariance, of
//                                        the two oldest frames of the window that lie K images apart (default 1: the oldest clone, each consecutive
//                                        edge at its most smoothed, just before it is marginalised) behind every frame, read in bulk from the
//                                        handle's edge ring of N records (default 256; System::record_edges_to); one line per record, stamped
//                                        with the two images it connects (format_edge: t_new t_old p q cov)
//                                        --landmarks: Updater::update's landmark cloud behind every updating frame (System::record_landmarks_to)
//                                        --landmark-cov: the 3 x 3 covariance of every cloud point, one line per point: t feat n_obs status p_w[3]
//                                          cov_w (6 upper) p_r[3] cov_r (6 upper) rho rho_sigma (System::record_landmark_cov_to); the --landmarks
//                                          file keeps its format
//                                        [--velocity FILE [--velocity-sigma S] [--velocity-gate]] [--standstill FILE]
//                                        --standstill: with Standstill.Enable: 1 in the settings (the device-side standstill detector and its
//                                        zero-velocity update behind every frame), one line per frame `t T disparity n_pairs flags gamma`, kept on the
//                                        host and written once at the end
//                                        --velocity: a CSV of `t_ns, vx, vy, vz` — the velocity in the IMU frame, e.g. from wheel encoders — fused on the
//                                        device (System::velocity) right behind the frame whose image stamp is nearest to t_ns, within half an image
//                                        period; at most one row per frame (the last one wins), rows that match no frame are counted and the count is
//                                        printed.  S: the standard deviation per axis in m/s (default 0.05); --velocity-gate: the 95 % chi-square gate
//                                        [--fix FILE [--fix-gate]]
//                                        --fix: absolute fixes, one per line `t kind values... sigmas... [lever]` (rvio_host.hpp parse_fixes: a world-frame
//                                        position, attitude or pose in the pose file's frame and convention, or the accelerometer at rest), each
//                                        linearised and fused on the device (System::fix_position / _attitude / _pose / _gravity) behind the first
//                                        frame whose image stamp is >= t, ahead of that frame's pose line — at THAT frame's state, not at t: the gap is
//                                        not bridged.  --fix-gate: the 95 % chi-square gate.  A malformed line is an error that names the line
//                                        [--fix-latency S]   (with --fix) the fixes arrive S seconds late, as real ones do: a row becomes available behind
//                                        the first frame whose image stamp is >= t + S and is fused AT ITS OWN t, against the pose the clone window
//                                        still holds for that time (System::fix_*_at -> rvio_hip_update_fix_past): a position interpolated between
//                                        the two frames around t, an attitude or pose at the nearest frame; a row older than the window by then is
//                                        dropped and counted, a gravity row is fused at the frame.  S: a finite number >= 0
//                                        [--rel FILE [--rel-gate]]
//                                        --rel: relative-pose measurements, one per line `t_new t_old kind values... sigmas... [lever]` (rvio_host.hpp
//                                        parse_rels: the delta pose of the IMU between two instants, as a wheel-odometry integrator, a scan matcher or
//                                        a loop closure inside the window gives it), each linearised and fused on the device (System::update_rel_at ->
//                                        rvio_hip_update_rel) behind the first frame whose image stamp is >= t_new, between the two frames of the clone
//                                        window nearest to its stamps; a row whose older stamp has left the window, or whose stamps fall onto one frame,
//                                        is dropped and counted.  --rel-gate: the 95 % chi-square gate.  A malformed line is an error that names the line
//                                        [--map FILE [--map-units px|norm] [--map-latency S] [--map-gate]]
//                                        --map: observations of known world points, one per line `t x y z u v sigma` (rvio_host.hpp parse_map: the
//                                        point in the filter's world frame, seen at (u, v) in the image stamped t), grouped by stamp; each group is
//                                        linearised and fused on the device (System::map_points_at -> rvio_hip_update_map, more than 8 points in
//                                        successive calls; --map-gate: every point behind its own 95 % chi-square gate, off by default like --fix-gate) behind the first frame whose image stamp is >=
//                                        t + S (--map-latency, default 0: matches arrive late), at the frame of the window nearest to t.  A stamp
//                                        older than the window is reported and skipped.  --map-units: px (raw pixels, the default) or norm
//                                        (undistorted normalised coordinates)
//   rvio_replay --check-settings <settings.yaml>        print the parsed configuration (no GPU needed)
//   rvio_replay --check-fix <fixes.txt>                 print the parsed fix file, one JSON object per fix (no GPU needed)
//   rvio_replay --check-fix-age <t0,t1,..> <t> [nearest] where a fix stamped t falls among the window's image stamps, newest first (no GPU needed)
//   rvio_replay --check-rel <rels.txt>                  print the parsed rel file, one JSON object per measurement (no GPU needed)
//   rvio_replay --check-rel-span <t0,t1,..> <t_new> <t_old>   which two frames of the window a pair of stamps means, stamps newest first (no GPU needed)
//   rvio_replay --check-map <map.txt>                   print the parsed map file, one JSON object per observation (no GPU needed)
//   rvio_replay --check-map-age <t0,t1,..> <t>          which frame of the window a map stamp means, stamps newest first (no GPU needed)
//   rvio_replay --check-map-split <n>                   the successive calls n points are fused in (no GPU needed)
//   rvio_replay --check-dataset <asl_root>              print what the dataset reader found (no GPU needed)
//   rvio_replay --check-image <file.png|.pgm>           decode one image and print its size and checksum (no GPU needed)
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rvio_host.hpp"

using namespace rvio;

static int check_settings(const char* path) {
    Settings s; std::string err;
    if (!read_settings(path, &s, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    for (const std::string& k : s.missing) std::fprintf(stderr, "settings: %s is missing (upstream would read 0); the EuRoC default is used\n", k.c_str());
    const rvio_config& c = s.cfg;
    std::printf("{\"imu_rate\": %.17g, \"sigma_g\": %.17g, \"sigma_wg\": %.17g, \"sigma_a\": %.17g, \"sigma_wa\": %.17g, \"gravity\": %.17g, "
                "\"small_angle\": %.17g, \"width\": %d, \"height\": %d, \"fx\": %.9g, \"fy\": %.9g, \"cx\": %.9g, \"cy\": %.9g, "
                "\"k1\": %.9g, \"k2\": %.9g, \"p1\": %.9g, \"p2\": %.9g, \"k3\": %.9g, \"sigma_px\": %.9g, \"sigma_py\": %.9g, \"fisheye\": %d, "
                "\"n_features\": %d, \"max_track_len\": %d, \"min_track_len\": %d, \"min_dist\": %.9g, \"qual_lvl\": %.9g, \"block_x\": %.9g, "
                "\"block_y\": %.9g, \"enable_equalizer\": %d, \"use_sampson\": %d, \"inlier_thr\": %.17g, \"ini_thr_angle\": %.17g, "
                "\"ini_thr_displ\": %.17g, \"ini_enable_alignment\": %d, \"cam_time_offset\": %.17g, \"record_outputs\": %d, \"is_rgb\": %d, \"T_bc\": [",
                c.imu_rate, c.sigma_g, c.sigma_wg, c.sigma_a, c.sigma_wa, c.gravity, c.small_angle, c.width, c.height, c.fx, c.fy, c.cx, c.cy,
                c.k1, c.k2, c.p1, c.p2, c.k3, c.sigma_px, c.sigma_py, c.fisheye, c.n_features, c.max_track_len, c.min_track_len, c.min_dist,
                c.qual_lvl, c.block_x, c.block_y, c.enable_equalizer, c.use_sampson, c.inlier_thr, c.ini_thr_angle, c.ini_thr_displ,
                c.ini_enable_alignment, s.cam_time_offset, s.record_outputs, s.is_rgb);
    for (int i = 0; i < 16; ++i) std::printf("%s%.17g", i ? ", " : "", c.T_bc[i]);
    const rvio_standstill_config& z = s.standstill;   // Standstill.* (optional keys)
    std::printf("], \"standstill\": {\"enable\": %d, \"sigma_a\": %.17g, \"sigma_w\": %.17g, \"imu_thr\": %.17g, \"disp_thr_px\": %.17g, \"min_pairs\": %d, "
                "\"sigma_v\": %.17g, \"sigma_bg\": %.17g, \"bias_rows\": %d, \"gate\": %d}",
                s.standstill_enable, z.sigma_a, z.sigma_w, z.imu_thr, z.disp_thr_px, (int)z.min_pairs, z.sigma_v, z.sigma_bg, (int)z.bias_rows, (int)z.gate);
    std::printf(", \"meas\": {\"iterations\": %d, \"tolerance\": %.17g}", s.meas_iterations, s.meas_tolerance);   // Meas.* (optional keys)
    std::printf(", \"encoding\": \"%s\"}\n", s.encoding.c_str());
    return 0;
}

static int check_dataset(const char* root) {
    AslDataset d; std::string err;
    if (!read_asl(root, &d, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    std::printf("{\"images\": %zu, \"imu\": %zu", d.images.size(), d.imu.size());
    if (!d.images.empty()) std::printf(", \"t_first_image\": %.9f, \"first_image\": \"%s\"", d.images.front().first, d.images.front().second.c_str());
    if (d.imu.size() > 1) std::printf(", \"t_first_imu\": %.9f, \"dt1\": %.9f, \"w1\": [%.17g, %.17g, %.17g]", d.imu[0].t, d.imu[1].dt, d.imu[1].w[0], d.imu[1].w[1], d.imu[1].w[2]);
    std::printf("}\n");
    return 0;
}

// encoding: a ROS encoding name (Camera.Encoding), or nullptr: what follows from the file and the channel order
static int check_image(const char* path, bool is_rgb, const char* encoding) {
    ImageData im; std::string err;
    if (!read_image(path, &im, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    const int channels = im.channels, bits = im.bits;
    Settings s;
    s.is_rgb = is_rgb ? 1 : 0;
    if (encoding) {
        if (encoding_format(encoding) < 0) { std::fprintf(stderr, "unknown encoding '%s'\n", encoding); return 1; }
        s.encoding = encoding;
    }
    const int fmt = image_format(im, s, &err);
    if (fmt < 0 || !to_gray(&im, fmt, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    unsigned long long sum = 0, wsum = 0;
    for (size_t i = 0; i < im.px.size(); ++i) { sum += im.px[i]; wsum += (unsigned long long)im.px[i] * (i % 251 + 1); }
    std::printf("{\"width\": %d, \"height\": %d, \"channels\": %d, ", im.width, im.height, channels);
    if (bits != 8 || encoding) std::printf("\"bits\": %d, \"format\": %d, ", bits, fmt);   // (an 8-bit file without --encoding prints what it always printed)
    std::printf("\"sum\": %llu, \"wsum\": %llu}\n", sum, wsum);
    return 0;
}

// ---------------------------------------------------------------- --fix
static int check_fix(const char* path) {
    std::vector<FixRow> rows; std::string err;
    if (!read_fixes(path, &rows, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    for (const FixRow& r : rows) {
        std::printf("{\"t\": %.17g, \"kind\": %d, \"z\": [", r.t, r.kind);
        for (int i = 0; i < 7; ++i) std::printf("%s%.17g", i ? ", " : "", r.fix.z[i]);
        std::printf("], \"sigma\": [");
        for (int i = 0; i < 6; ++i) std::printf("%s%.17g", i ? ", " : "", r.fix.sigma[i]);
        std::printf("], \"lever\": [%.17g, %.17g, %.17g]}\n", r.fix.lever[0], r.fix.lever[1], r.fix.lever[2]);
    }
    return 0;
}

// --check-fix-age: resolve_fix_age on stamps given newest first
static int check_fix_age(const char* list, const char* t_arg, bool nearest) {
    std::vector<double> stamps;
    std::string flat = list;
    for (char& c : flat) if (c == ',') c = ' ';
    const char* p = flat.c_str();
    for (char* end = nullptr;; p = end) { const double v = std::strtod(p, &end); if (end == p) break; stamps.push_back(v); }
    const FixAge w = resolve_fix_age(stamps, std::atof(t_arg), !nearest);
    std::printf("{\"where\": %d, \"age\": %d, \"frac\": %.17g}\n", w.where, w.age, w.frac);
    return 0;
}
// ---------------------------------------------------------------- --rel
static int check_rel(const char* path) {
    std::vector<RelRow> rows; std::string err;
    if (!read_rels(path, &rows, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    for (const RelRow& r : rows) {
        std::printf("{\"t_new\": %.17g, \"t_old\": %.17g, \"kind\": %d, \"z\": [", r.t_new, r.t_old, r.kind);
        for (int i = 0; i < 7; ++i) std::printf("%s%.17g", i ? ", " : "", r.meas.z[i]);
        std::printf("], \"sigma\": [");
        for (int i = 0; i < 6; ++i) std::printf("%s%.17g", i ? ", " : "", r.meas.sigma[i]);
        std::printf("], \"lever\": [%.17g, %.17g, %.17g]}\n", r.meas.lever[0], r.meas.lever[1], r.meas.lever[2]);
    }
    return 0;
}
static std::vector<double> stamp_list(const char* list) {
    std::vector<double> stamps;
    std::string flat = list;
    for (char& c : flat) if (c == ',') c = ' ';
    const char* p = flat.c_str();
    for (char* end = nullptr;; p = end) { const double v = std::strtod(p, &end); if (end == p) break; stamps.push_back(v); }
    return stamps;
}
// ---------------------------------------------------------------- --map
static int check_map(const char* path) {
    std::vector<MapRow> rows; std::string err;
    if (!read_map(path, &rows, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    for (const MapRow& r : rows)
        std::printf("{\"t\": %.17g, \"p_w\": [%.17g, %.17g, %.17g], \"uv\": [%.17g, %.17g], \"sigma\": %.17g}\n", r.t, r.obs.p_w[0], r.obs.p_w[1], r.obs.p_w[2],
                    r.obs.uv[0], r.obs.uv[1], r.obs.sigma);
    return 0;
}
static int check_map_split(const char* n) {
    std::printf("[");
    bool first = true;
    for (const std::pair<int, int>& c : map_calls(std::atoi(n))) { std::printf("%s[%d, %d]", first ? "" : ", ", c.first, c.second); first = false; }
    std::printf("]\n");
    return 0;
}
// --check-rel-span: resolve_rel_span on stamps given newest first
static int check_rel_span(const char* list, const char* t_new, const char* t_old) {
    const RelSpan w = resolve_rel_span(stamp_list(list), std::atof(t_new), std::atof(t_old));
    std::printf("{\"ok\": %d, \"age_new\": %d, \"age_old\": %d}\n", w.ok ? 1 : 0, w.age_new, w.age_old);
    return 0;
}
// --check-map-age: resolve_map_age on stamps given newest first
static int check_map_age(const char* list, const char* t) {
    const MapAge w = resolve_map_age(stamp_list(list), std::atof(t));
    std::printf("{\"ok\": %d, \"age\": %d}\n", w.ok ? 1 : 0, w.age);
    return 0;
}
// --fix-latency: seconds, finite and >= 0
static bool parse_latency(const char* arg, double* out) {
    char* end = nullptr;
    const double v = std::strtod(arg, &end);
    if (end == arg || *end != 0 || !std::isfinite(v) || v < 0) return false;
    *out = v;
    return true;
}

// ---------------------------------------------------------------- --velocity
struct VelocityRows {
    std::vector<int> has;                 // per image of the dataset: a row was matched to it
    std::vector<double> v;                // ... and its velocity, 3 per image
    long rows = 0, unmatched = 0, applied = 0;
    double sigma = 0.05; bool gate = false;
};
// lines of `t_ns, vx, vy, vz` ('#' lines and a header line without a leading digit are skipped); the image whose stamp is nearest, if that is
// within half the mean image period, takes the row
static bool read_velocity(const char* path, const AslDataset& d, VelocityRows* out, std::string* err) {
    std::ifstream in(path);
    if (!in) { *err = std::string("cannot read ") + path; return false; }
    const size_t N = d.images.size();
    out->has.assign(N, 0); out->v.assign(3 * N, 0.0);
    const double period = N > 1 ? (d.images.back().first - d.images.front().first) / (double)(N - 1) : 0.0;
    std::string line;
    while (std::getline(in, line)) {
        size_t b = line.find_first_not_of(" \t\r");
        if (b == std::string::npos || line[b] == '#' || !(line[b] >= '0' && line[b] <= '9')) continue;
        long long ns = 0; double v[3];
        if (std::sscanf(line.c_str() + b, "%lld , %lf , %lf , %lf", &ns, &v[0], &v[1], &v[2]) != 4) { *err = std::string(path) + ": not `t_ns, vx, vy, vz`: " + line; return false; }
        ++out->rows;
        const double t = (double)(ns / 1000000000LL) + 1e-9 * (double)(ns % 1000000000LL);
        auto it = std::lower_bound(d.images.begin(), d.images.end(), t, [](const std::pair<double, std::string>& im, double tt) { return im.first < tt; });
        size_t k = (size_t)(it - d.images.begin());
        if (k == N || (k > 0 && t - d.images[k - 1].first <= d.images[k].first - t)) k = k > 0 ? k - 1 : k;
        if (N == 0 || std::fabs(d.images[k].first - t) > 0.5 * period) { ++out->unmatched; continue; }
        out->has[k] = 1;
        for (int i = 0; i < 3; ++i) out->v[3 * k + i] = v[i];
    }
    return true;
}
// behind the frame of image k, if the filter processed it
static int apply_velocity(System& sys, VelocityRows* vr, size_t k) {
    if (!vr || k >= vr->has.size() || !vr->has[k]) return 0;
    if (sys.velocity(&vr->v[3 * k], vr->sigma, vr->gate) < 0) return -1;
    ++vr->applied;
    return 0;
}
static void print_velocity(const VelocityRows& vr) {
    std::fprintf(stderr, "rvio_replay: velocity: %ld rows, %ld applied, %ld matched no frame\n", vr.rows, vr.applied, vr.unmatched);
}

// ---------------------------------------------------------------- replay passes
struct FrameDump {            // what the device holds behind a frame (read with every stream drained)
    rvio_frame_info info{};
    int n_feat = 0;
    std::vector<unsigned char> types;
    std::vector<int32_t> len;
    std::vector<float> meas;
};
struct PassOptions {
    bool sync_every_frame = false;   // rvio_hip_sync behind every MonoVIO call (the reference pacing: nothing overlaps)
    long stall_seed = -1;            // >= 0: sleeping kernels on random streams in front of random frames (rvio_hip_debug_stall)
    int noise_wgs = 0;               // > 0: that many workgroups of HBM / L2 / LDS traffic beside every fourth frame (rvio_hip_debug_noise)
    long dump_at = -1;               // filtered-frame index behind which the streams are drained and the hand-over is read back
    long max_frames = -1;
    const char* landmarks = nullptr; // System::record_landmarks_to
    const char* landmark_cov = nullptr; // System::record_landmark_cov_to
    const char* odometry = nullptr;  // System::record_odometry_to
    int odometry_ring = 256;
    const char* smoothed = nullptr;  // System::record_smoothed_to
    int smoothed_lag = -1, smoothed_ring = 256;
    const char* edges = nullptr;     // System::record_edges_to
    int edges_span = 1, edges_ring = 256;
    const char* imu_odometry = nullptr;  // System::record_imu_odometry_to
    int imu_odometry_ring = 4096;
    bool imu_odometry_cov = false;
    VelocityRows* velocity = nullptr;    // --velocity
    const std::vector<FixRow>* fixes = nullptr;   // --fix
    bool fix_gate = false;
    double fix_latency = -1.0;           // --fix-latency (< 0: not given)
    const std::vector<RelRow>* rels = nullptr;    // --rel
    bool rel_gate = false;
    const std::vector<MapRow>* maps = nullptr;    // --map
    int map_units = RVIO_MAP_PIXELS;
    double map_latency = 0.0;
    bool map_gate = false;
};
static bool dump_frame(System& sys, const rvio_config& c, FrameDump* d) {
    rvio_hip* h = sys.handle();
    const int Fu = (c.n_features + 1) / 2, ML = c.max_track_len;
    if (rvio_hip_sync(h) != RVIO_OK) return false;
    if (rvio_hip_get_frame_info(h, &d->info) != RVIO_OK) return false;
    d->types.assign(Fu, 0); d->len.assign(Fu, 0); d->meas.assign((size_t)Fu * ML * 2, 0.f);
    int32_t nf = 0;
    if (rvio_hip_get_tracks(h, &nf, d->types.data(), d->len.data(), d->meas.data()) != RVIO_OK) return false;
    d->n_feat = nf;
    return true;
}
// one pass over the dataset with a fresh System; poses of the filtered frames, optionally the dump of every frame (sync_every_frame) or of one
static int run_pass(const Settings& s, const AslDataset& d, int device, const PassOptions& o, std::vector<PoseLine>* poses,
                    std::vector<FrameDump>* dumps, double* ms_per_call, int* flags, std::string* err) {
    System sys(s, device);
    if (!sys.ok()) { *err = sys.error(); return 1; }
    if (o.landmarks && !sys.record_landmarks_to(o.landmarks)) { *err = sys.error(); return 1; }
    if (o.landmark_cov && !sys.record_landmark_cov_to(o.landmark_cov)) { *err = sys.error(); return 1; }
    if (o.odometry && !sys.record_odometry_to(o.odometry, o.odometry_ring)) { *err = sys.error(); return 1; }
    if (o.smoothed && !sys.record_smoothed_to(o.smoothed, o.smoothed_lag < 0 ? s.cfg.max_track_len - 1 : o.smoothed_lag, o.smoothed_ring)) { *err = sys.error(); return 1; }
    if (o.edges && !sys.record_edges_to(o.edges, s.cfg.max_track_len - 1 - o.edges_span, s.cfg.max_track_len - 1, o.edges_ring)) { *err = sys.error(); return 1; }
    if (o.imu_odometry && !sys.record_imu_odometry_to(o.imu_odometry, o.imu_odometry_ring, o.imu_odometry_cov)) { *err = sys.error(); return 1; }
    if (o.fixes) sys.queue_fixes(*o.fixes, o.fix_gate, o.fix_latency);
    if (o.rels) sys.queue_rels(*o.rels, o.rel_gate);
    if (o.maps) sys.queue_map(*o.maps, o.map_units, o.map_latency, o.map_gate);
    size_t ii = 0;
    long n_images = 0, n_frames = 0;
    double t_filter = 0;
    unsigned long long lcg = 0x9e3779b97f4a7c15ull ^ (unsigned long long)(o.stall_seed + 1);
    auto rnd = [&](unsigned mod) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((lcg >> 33) % mod); };
    size_t image_k = (size_t)-1;
    for (const auto& im : d.images) {
        ++image_k;
        if (o.max_frames >= 0 && n_images >= o.max_frames) break;
        while (ii < d.imu.size() && (d.imu[ii].t <= im.first + s.cam_time_offset || (ii > 0 && d.imu[ii - 1].t <= im.first + s.cam_time_offset))) sys.PushImuData(d.imu[ii++]);
        ImageData img;
        if (!read_image(im.second, &img, err)) return 1;
        img.t = im.first;
        sys.PushImageData(std::move(img));
        ++n_images;
        if (o.stall_seed >= 0 && sys.is_ready())
            for (unsigned k = rnd(3); k > 0; --k) rvio_hip_debug_stall(sys.handle(), (int)rnd(4), 30 + (int)rnd(870));
        if (o.noise_wgs > 0 && sys.is_ready() && n_images % 4 == 0) rvio_hip_debug_noise(sys.handle(), o.noise_wgs, 1500);
        PoseLine p;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = sys.MonoVIO(&p);
        t_filter += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc < 0) { *err = sys.error(); return 1; }
        if (rc == 1) {
            poses->push_back(p);
            if (apply_velocity(sys, o.velocity, image_k) < 0) { *err = sys.error(); return 1; }
            if (o.sync_every_frame || o.dump_at == n_frames) {
                FrameDump fd;
                if (!dump_frame(sys, s.cfg, &fd)) { *err = rvio_hip_last_error(sys.handle()); return 1; }
                if (dumps) dumps->push_back(std::move(fd));
            }
            ++n_frames;
            if (o.dump_at >= 0 && n_frames > o.dump_at) break;
        }
    }
    if (sys.flush_odometry() < 0 || sys.flush_smoothed() < 0 || sys.flush_edges() < 0 || sys.flush_imu_odometry() < 0) { *err = sys.error(); return 1; }
    if (ms_per_call) *ms_per_call = n_images ? 1e3 * t_filter / n_images : 0.0;
    if (flags) *flags = sys.device_flags();
    return 0;
}
static double pose_diff(const PoseLine& a, const PoseLine& b) {
    double m = 0;
    for (int i = 0; i < 3; ++i) m = std::max(m, std::fabs(a.p[i] - b.p[i]));
    const double sa = a.q[3] < 0 ? -1 : 1, sb = b.q[3] < 0 ? -1 : 1;
    for (int i = 0; i < 4; ++i) m = std::max(m, std::fabs(sa * a.q[i] - sb * b.q[i]));
    return m;
}
// which HIP runtime this process ended up with (a Python process loads torch's bundled copy first; this binary takes /opt/rocm's through
// the library's DT_NEEDED) — resolved from the process image, no link-time dependency of the host on the runtime
static void print_runtime() {
    typedef int (*ver_fn)(int*);
    int rt = 0, drv = 0;
    const char* path = "?";
    if (ver_fn f = (ver_fn)dlsym(RTLD_DEFAULT, "hipRuntimeGetVersion")) {
        (void)f(&rt);
        Dl_info di{};
        if (dladdr((void*)f, &di) && di.dli_fname) path = di.dli_fname;
    }
    if (ver_fn f = (ver_fn)dlsym(RTLD_DEFAULT, "hipDriverGetVersion")) (void)f(&drv);
    std::fprintf(stderr, "rvio_replay: HIP runtime %d, driver %d, libamdhip64 = %s, RVIO_PARANOID=%s\n", rt, drv, path,
                 getenv("RVIO_PARANOID") ? getenv("RVIO_PARANOID") : "");
}
// --selfcheck: the pipelined replay against the SAME binary's synchronised pass (rvio_hip_sync behind every frame), pose by pose and bit for
// bit; on a mismatch the pipelined pass is repeated up to the first differing frame, drained there, and the first table that differs —
// front-end counters, hand-over count / types / lengths / measurements — is printed beside the synchronised pass's.  Exit status 3.
static int selfcheck(const Settings& s, const AslDataset& d, int device, long max_frames, long stall_seed, int noise_wgs) {
    std::string err;
    std::vector<PoseLine> ref, got;
    std::vector<FrameDump> dref;
    PassOptions o; o.max_frames = max_frames;
    PassOptions os = o; os.sync_every_frame = true;
    if (run_pass(s, d, device, os, &ref, &dref, nullptr, nullptr, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    PassOptions op = o; op.stall_seed = stall_seed; op.noise_wgs = noise_wgs;
    int flags = 0;
    if (run_pass(s, d, device, op, &got, nullptr, nullptr, &flags, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    long first = -1; double worst = 0;
    for (size_t i = 0; i < std::min(ref.size(), got.size()); ++i) {
        const double df = pose_diff(ref[i], got[i]);
        if (df > 0 && first < 0) first = (long)i;
        worst = std::max(worst, df);
    }
    if (ref.size() != got.size() && first < 0) first = (long)std::min(ref.size(), got.size());
    std::fprintf(stderr, "rvio_replay --selfcheck: %zu / %zu filtered frames (synchronised / pipelined%s), max |pose diff| %.3e, first differing frame %ld, device flags %d\n",
                 ref.size(), got.size(), stall_seed >= 0 ? " with stalled queues" : "", worst, first, flags);
    if (first < 0) return 0;
    std::vector<PoseLine> again; std::vector<FrameDump> dgot;
    PassOptions od = op; od.dump_at = first;
    if (run_pass(s, d, device, od, &again, &dgot, nullptr, nullptr, &err) || dgot.empty() || (size_t)first >= dref.size()) {
        std::fprintf(stderr, "  (could not re-run up to frame %ld: %s)\n", first, err.c_str());
        return 3;
    }
    const FrameDump &a = dref[first], &b = dgot[0];
    std::fprintf(stderr, "  frame %ld           synchronised   pipelined\n", first);
#define ROW(name, f) std::fprintf(stderr, "  %-18s %12d %12d%s\n", name, (int)a.f, (int)b.f, a.f != b.f ? "   <--" : "")
    ROW("n_tracked_in", info.n_tracked_in); ROW("n_klt_ok", info.n_klt_ok); ROW("n_ransac_inliers", info.n_ransac_inliers); ROW("ransac_winner", info.ransac_winner);
    ROW("n_feat_update", info.n_feat_update); ROW("n_tracked_out", info.n_tracked_out); ROW("n_feat_accepted", info.n_feat_accepted); ROW("n_rows", info.n_rows);
    ROW("updated", info.updated); ROW("hand-over n_feat", n_feat);
#undef ROW
    const int ML = s.cfg.max_track_len;
    for (int f = 0; f < std::min(a.n_feat, b.n_feat); ++f) {
        bool same = a.types[f] == b.types[f] && a.len[f] == b.len[f];
        for (int k = 0; same && k < 2 * a.len[f]; ++k) same = a.meas[(size_t)f * ML * 2 + k] == b.meas[(size_t)f * ML * 2 + k];
        if (!same) { std::fprintf(stderr, "  hand-over feature %d differs: type %c / %c, len %d / %d\n", f, a.types[f], b.types[f], a.len[f], b.len[f]); break; }
    }
    return 3;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "--check-settings")) return check_settings(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "--check-dataset")) return check_dataset(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "--check-fix")) return check_fix(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "--check-fix-age")) return check_fix_age(argv[2], argv[3], argc >= 5 && !std::strcmp(argv[4], "nearest"));
    if (argc >= 3 && !std::strcmp(argv[1], "--check-rel")) return check_rel(argv[2]);
    if (argc >= 5 && !std::strcmp(argv[1], "--check-rel-span")) return check_rel_span(argv[2], argv[3], argv[4]);
    if (argc >= 3 && !std::strcmp(argv[1], "--check-map")) return check_map(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "--check-map-age")) return check_map_age(argv[2], argv[3]);
    if (argc >= 3 && !std::strcmp(argv[1], "--check-map-split")) return check_map_split(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "--check-image")) {   // --check-image FILE [--bgr] [--encoding NAME]
        bool rgb = true; const char* enc = nullptr;
        for (int i = 3; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--bgr")) rgb = false;
            else if (!std::strcmp(argv[i], "--encoding") && i + 1 < argc) enc = argv[++i];
        }
        return check_image(argv[2], rgb, enc);
    }
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <settings.yaml> <asl_root> [<poses_out.dat>] [--device N] [--max-frames K] [--record-dir DIR] [--record]\n"
                             "          [--landmarks FILE] [--landmark-cov FILE] [--odometry FILE] [--odometry-ring N] [--smoothed FILE] [--smoothed-lag L] [--smoothed-ring N] [--edges FILE] [--edges-span K] [--edges-ring N] [--imu-odometry FILE] [--imu-odometry-ring N] [--imu-odometry-cov] [--sync-every-frame] [--stall-seed S] [--noise WGS] [--selfcheck]\n"
                             "          [--velocity FILE] [--velocity-sigma S] [--velocity-gate] [--standstill FILE] [--fix FILE] [--fix-gate] [--fix-latency S]\n"
                             "          [--rel FILE] [--rel-gate] [--map FILE] [--map-units px|norm] [--map-latency S] [--map-gate]\n"
                             "          [--meas-iters N] [--meas-tol T]\n", argv[0]);
        return 2;
    }
    const char* out_path = nullptr;
    int device = 0; long max_frames = -1, stall_seed = -1;
    const char* landmarks = nullptr;
    const char* landmark_cov = nullptr;
    const char* odometry = nullptr; int odometry_ring = 256;
    const char* smoothed = nullptr; int smoothed_lag = -1, smoothed_ring = 256;
    const char* edges = nullptr; int edges_span = 1, edges_ring = 256;
    const char* imu_odometry = nullptr; int imu_odometry_ring = 4096; bool imu_odometry_cov = false;
    const char* velocity = nullptr; double velocity_sigma = 0.05; bool velocity_gate = false;
    const char* standstill = nullptr;
    const char* fix = nullptr; bool fix_gate = false; double fix_latency = -1.0;
    const char* rel = nullptr; bool rel_gate = false;
    const char* map = nullptr; int map_units = RVIO_MAP_PIXELS; double map_latency = 0.0; bool map_gate = false;
    int meas_iters = 0; double meas_tol = -1.0;   // (0 / -1: not given, the settings' Meas.* hold)
    const char* record_dir = "."; bool force_record = false, sync_every = false, self = false; int noise_wgs = 0;
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--max-frames") && i + 1 < argc) max_frames = std::atol(argv[++i]);
        else if (!std::strcmp(argv[i], "--record-dir") && i + 1 < argc) record_dir = argv[++i];   // where INI.RecordOutputs: 1 writes its two files
        else if (!std::strcmp(argv[i], "--record")) force_record = true;                          // as if the settings said INI.RecordOutputs: 1
        else if (!std::strcmp(argv[i], "--sync-every-frame")) sync_every = true;                   // rvio_hip_sync behind every frame (A/B of the pipelining)
        else if (!std::strcmp(argv[i], "--stall-seed") && i + 1 < argc) stall_seed = std::atol(argv[++i]);   // sleeping kernels on random streams (A/B of the ordering)
        else if (!std::strcmp(argv[i], "--noise") && i + 1 < argc) noise_wgs = std::atoi(argv[++i]);         // a loaded chip beside the replay (A/B of timing inside kernels)
        else if (!std::strcmp(argv[i], "--landmark-cov") && i + 1 < argc) landmark_cov = argv[++i];   // the covariance records of every cloud, one point per line
        else if (!std::strcmp(argv[i], "--landmarks") && i + 1 < argc) landmarks = argv[++i];   // the landmark cloud of every update, one point per line
        else if (!std::strcmp(argv[i], "--odometry") && i + 1 < argc) odometry = argv[++i];     // one line per frame: pose, velocity, pose covariance (read in bulk from the ring)
        else if (!std::strcmp(argv[i], "--odometry-ring") && i + 1 < argc) odometry_ring = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--smoothed") && i + 1 < argc) smoothed = argv[++i];     // one line per record: pose and pose covariance of the frame L images back (read in bulk from the smoothed ring)
        else if (!std::strcmp(argv[i], "--smoothed-lag") && i + 1 < argc) smoothed_lag = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--smoothed-ring") && i + 1 < argc) smoothed_ring = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--edges") && i + 1 < argc) edges = argv[++i];           // one line per record: the edge between the two oldest frames K images apart (read in bulk from the edge ring)
        else if (!std::strcmp(argv[i], "--edges-span") && i + 1 < argc) edges_span = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--edges-ring") && i + 1 < argc) edges_ring = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--imu-odometry") && i + 1 < argc) imu_odometry = argv[++i];   // one line per IMU sample: pose and velocity (read in bulk from the IMU-rate ring)
        else if (!std::strcmp(argv[i], "--imu-odometry-ring") && i + 1 < argc) imu_odometry_ring = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--imu-odometry-cov")) imu_odometry_cov = true;   // ... and the covariance of each sample's pose and velocity behind it
        else if (!std::strcmp(argv[i], "--selfcheck")) self = true;
        else if (!std::strcmp(argv[i], "--velocity") && i + 1 < argc) velocity = argv[++i];   // `t_ns, vx, vy, vz` rows fused behind the nearest frame (System::velocity)
        else if (!std::strcmp(argv[i], "--velocity-sigma") && i + 1 < argc) velocity_sigma = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--velocity-gate")) velocity_gate = true;
        else if (!std::strcmp(argv[i], "--standstill") && i + 1 < argc) standstill = argv[++i];   // one line per frame: t T disparity n_pairs flags gamma (needs Standstill.Enable: 1)
        else if (!std::strcmp(argv[i], "--fix") && i + 1 < argc) fix = argv[++i];   // `t kind values... sigmas... [lever]` lines fused behind the first frame at or past t (System::fix_*)
        else if (!std::strcmp(argv[i], "--fix-gate")) fix_gate = true;
        else if (!std::strcmp(argv[i], "--fix-latency")) {   // seconds the fixes arrive late: fused at their own stamp (System::fix_*_at)
            if (i + 1 >= argc || !parse_latency(argv[i + 1], &fix_latency)) { std::fprintf(stderr, "--fix-latency takes seconds, a finite number >= 0\n"); return 1; }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--rel") && i + 1 < argc) rel = argv[++i];   // `t_new t_old kind values... sigmas... [lever]` lines fused behind the first frame at or past t_new (System::update_rel_at)
        else if (!std::strcmp(argv[i], "--rel-gate")) rel_gate = true;
        else if (!std::strcmp(argv[i], "--map") && i + 1 < argc) map = argv[++i];   // `t x y z u v sigma` lines, grouped by stamp, fused at the frame nearest to t (System::map_points_at)
        else if (!std::strcmp(argv[i], "--map-gate")) map_gate = true;
        else if (!std::strcmp(argv[i], "--meas-iters") && i + 1 < argc) {   // the --fix / --rel / --map measurements relinearised N times on the device (rvio_hip_set_meas_iterations)
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end != 0 || v < 1 || v > RVIO_MEAS_MAX_ITERS) { std::fprintf(stderr, "--meas-iters takes an integer in 1 .. %d, not '%s'\n", RVIO_MEAS_MAX_ITERS, argv[i]); return 1; }
            meas_iters = (int)v;
        }
        else if (!std::strcmp(argv[i], "--meas-tol") && i + 1 < argc) {
            char* end = nullptr;
            meas_tol = std::strtod(argv[++i], &end);
            if (end == argv[i] || *end != 0 || !std::isfinite(meas_tol) || meas_tol < 0) { std::fprintf(stderr, "--meas-tol takes a finite number >= 0, not '%s'\n", argv[i]); return 1; }
        }
        else if (!std::strcmp(argv[i], "--map-units") && i + 1 < argc) {
            ++i;
            if (!std::strcmp(argv[i], "px")) map_units = RVIO_MAP_PIXELS;
            else if (!std::strcmp(argv[i], "norm")) map_units = RVIO_MAP_NORMALISED;
            else { std::fprintf(stderr, "--map-units takes px or norm, not '%s'\n", argv[i]); return 1; }
        }
        else if (!std::strcmp(argv[i], "--map-latency") && i + 1 < argc) {
            char* end = nullptr;
            map_latency = std::strtod(argv[++i], &end);
            if (end == argv[i] || *end != 0 || !std::isfinite(map_latency) || map_latency < 0) { std::fprintf(stderr, "--map-latency takes a finite number >= 0, not '%s'\n", argv[i]); return 1; }
        }
        else out_path = argv[i];
    }
    if (fix_latency >= 0 && !fix) { std::fprintf(stderr, "--fix-latency needs --fix FILE\n"); return 1; }
    Settings s; std::string err;
    if (!read_settings(argv[1], &s, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }   // System.cc:54-58: exit(-1)
    for (const std::string& k : s.missing) std::fprintf(stderr, "settings: %s is missing (upstream would read 0); the EuRoC default is used\n", k.c_str());
    AslDataset d;
    if (!read_asl(argv[2], &d, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    VelocityRows vrows; VelocityRows* vr = nullptr;
    if (velocity) {
        if (!(velocity_sigma > 0)) { std::fprintf(stderr, "--velocity-sigma must be > 0\n"); return 1; }
        if (self) { std::fprintf(stderr, "--velocity and --selfcheck do not combine\n"); return 1; }
        if (!read_velocity(velocity, d, &vrows, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        vrows.sigma = velocity_sigma; vrows.gate = velocity_gate;
        vr = &vrows;
    }
    std::vector<FixRow> fixes;
    if (fix) {
        if (self) { std::fprintf(stderr, "--fix and --selfcheck do not combine\n"); return 1; }
        if (!read_fixes(fix, &fixes, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    }
    std::vector<RelRow> rels;
    if (rel) {
        if (self) { std::fprintf(stderr, "--rel and --selfcheck do not combine\n"); return 1; }
        if (!read_rels(rel, &rels, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    }
    std::vector<MapRow> maps;
    if (map) {
        if (self) { std::fprintf(stderr, "--map and --selfcheck do not combine\n"); return 1; }
        if (!read_map(map, &maps, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    }
    if (meas_iters) s.meas_iterations = meas_iters;   // (the command line overrides the settings; System's constructor hands them to the library)
    if (meas_tol >= 0) s.meas_tolerance = meas_tol;
    print_runtime();
    if (self) return selfcheck(s, d, device, max_frames, stall_seed, noise_wgs);
    if (sync_every || stall_seed >= 0 || noise_wgs > 0) {   // the plain replay with one of the two A/B pacings
        std::vector<PoseLine> poses; double ms = 0; int flags = 0;
        PassOptions o; o.max_frames = max_frames; o.sync_every_frame = sync_every; o.stall_seed = stall_seed; o.noise_wgs = noise_wgs; o.landmarks = landmarks; o.landmark_cov = landmark_cov; o.odometry = odometry; o.odometry_ring = odometry_ring; o.smoothed = smoothed; o.smoothed_lag = smoothed_lag; o.smoothed_ring = smoothed_ring; o.edges = edges; o.edges_span = edges_span; o.edges_ring = edges_ring; o.imu_odometry = imu_odometry; o.imu_odometry_ring = imu_odometry_ring; o.imu_odometry_cov = imu_odometry_cov; o.velocity = vr; if (fix) { o.fixes = &fixes; o.fix_gate = fix_gate; o.fix_latency = fix_latency; } if (rel) { o.rels = &rels; o.rel_gate = rel_gate; } if (map) { o.maps = &maps; o.map_units = map_units; o.map_latency = map_latency; o.map_gate = map_gate; }
        if (run_pass(s, d, device, o, &poses, nullptr, &ms, &flags, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        if (out_path) { std::ofstream out(out_path); if (!out) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; } for (const PoseLine& p : poses) out << format_pose(p); }
        std::fprintf(stderr, "rvio_replay: %zu filtered frames, %.3f ms per MonoVIO call, device flags %d\n", poses.size(), ms, flags);
        if (vr) print_velocity(*vr);
        return 0;   // (the pass has printed nothing about --fix: its System is gone)
    }
    System sys(s, device);
    if (!sys.ok()) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (!sys.record_to(record_dir, force_record)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (landmarks && !sys.record_landmarks_to(landmarks)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (landmark_cov && !sys.record_landmark_cov_to(landmark_cov)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (odometry && !sys.record_odometry_to(odometry, odometry_ring)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (smoothed && !sys.record_smoothed_to(smoothed, smoothed_lag < 0 ? s.cfg.max_track_len - 1 : smoothed_lag, smoothed_ring)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (edges && !sys.record_edges_to(edges, s.cfg.max_track_len - 1 - edges_span, s.cfg.max_track_len - 1, edges_ring)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (imu_odometry && !sys.record_imu_odometry_to(imu_odometry, imu_odometry_ring, imu_odometry_cov)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (standstill && !sys.record_standstill_to(standstill)) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    if (fix) sys.queue_fixes(fixes, fix_gate, fix_latency);
    if (rel) sys.queue_rels(rels, rel_gate);
    if (map) sys.queue_map(maps, map_units, map_latency, map_gate);
    std::ofstream out;
    if (out_path) { out.open(out_path); if (!out) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; } }

    size_t ii = 0;
    long n_frames = 0, n_images = 0;
    double t_filter = 0;
    size_t image_k = (size_t)-1;
    for (const auto& im : d.images) {
        ++image_k;
        if (max_frames >= 0 && n_images >= max_frames) break;
        // IMU callbacks that precede this image (plus one sample beyond it, so that GetMeasurements sees enough data)
        while (ii < d.imu.size() && (d.imu[ii].t <= im.first + s.cam_time_offset || (ii > 0 && d.imu[ii - 1].t <= im.first + s.cam_time_offset))) sys.PushImuData(d.imu[ii++]);
        ImageData img;
        if (!read_image(im.second, &img, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        img.t = im.first;
        sys.PushImageData(std::move(img));
        ++n_images;
        PoseLine p;
        const auto t0 = std::chrono::steady_clock::now();
        // (with --odometry and no pose file nobody reads the pose line: the frame stays in flight, the ring is read in bulk)
        const int rc = sys.MonoVIO(odometry && !out.is_open() ? nullptr : &p);
        t_filter += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc < 0) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
        if (rc == 1) { ++n_frames; if (out.is_open()) out << format_pose(p); }
        if (rc == 1 && apply_velocity(sys, vr, image_k) < 0) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    }
    if (sys.flush_odometry() < 0 || sys.flush_smoothed() < 0 || sys.flush_edges() < 0 || sys.flush_imu_odometry() < 0 || sys.flush_standstill() < 0) { std::fprintf(stderr, "%s\n", sys.error().c_str()); return 1; }
    std::fprintf(stderr, "rvio_replay: %ld images, %ld filtered frames, %.3f ms per MonoVIO call (host wall clock, pose read-back included)\n",
                 n_images, n_frames, n_images ? 1e3 * t_filter / n_images : 0.0);
    if (vr) print_velocity(*vr);
    if (fix && fix_latency < 0) std::fprintf(stderr, "rvio_replay: fix: %zu rows, %ld applied\n", fixes.size(), sys.fixes_applied());
    if (fix && fix_latency >= 0) std::fprintf(stderr, "rvio_replay: fix: %zu rows, %ld fused, %ld older than the window and dropped (latency %g s)\n", fixes.size(), sys.fixes_applied() - sys.fixes_dropped(), sys.fixes_dropped(), fix_latency);
    if (rel) std::fprintf(stderr, "rvio_replay: rel: %zu rows, %ld fused, %ld outside the window or on one frame and dropped\n", rels.size(), sys.rels_applied() - sys.rels_dropped(), sys.rels_dropped());
    if (map) {
        for (double t : sys.map_skipped_stamps()) std::fprintf(stderr, "rvio_replay: map: the group stamped %.9f is older than the clone window: skipped\n", t);
        std::fprintf(stderr, "rvio_replay: map: %zu rows, %ld groups, %ld applied, %ld outside the window and skipped\n", maps.size(), sys.map_groups_applied(),
                     sys.map_groups_applied() - sys.maps_skipped(), sys.maps_skipped());
    }
    if ((fix || rel || map) && (s.meas_iterations != 1 || s.meas_tolerance != 0.0)) {
        rvio_meas_iter it;
        if (sys.last_meas_iter(&it))
            std::fprintf(stderr, "rvio_replay: meas-iters: at most %d passes, tolerance %g; the last measurement took %d, last step %.3e, converged %d, gamma of pass 0 %.6g\n",
                         s.meas_iterations, s.meas_tolerance, (int)it.iterations, it.step, (int)it.converged, it.gamma0);
        else std::fprintf(stderr, "rvio_replay: meas-iters: no measurement was fused (%s)\n", sys.error().c_str());
    }
    // anything only the device saw (0 in every test and bench run): said out loud, the poses above are suspect if it is not 0
    const int flags = sys.device_flags();
    if (flags) std::fprintf(stderr, "rvio_replay: DEVICE-SIDE FLAGS %d (1 singular pivot in the solve, 2 a track the window cannot hold was dropped, "
                                    "4 a stage counter timed out, 8 non-positive gate pivot)%s%s\n", flags, flags < 0 ? ": " : "", flags < 0 ? sys.error().c_str() : "");
    return 0;
}
