// host/rvio_host.cpp — see rvio_host.hpp.  No ROS / OpenCV / Eigen; zlib for PNG.
#include "rvio_host.hpp"
#include "../r-vio_amd/csrc/raw.h"   // the arithmetic of the device's raw-sensor gray conversion, as the kernels compile it

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

namespace rvio {

// ------------------------------------------------------------------ settings (OpenCV-YAML 1.0 subset)
namespace {
std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && std::isspace((unsigned char)s[a])) ++a;
    while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}
std::string strip_comment(const std::string& s) {
    const size_t p = s.find('#');
    return p == std::string::npos ? s : s.substr(0, p);
}
struct Yaml {
    std::map<std::string, double> num;
    std::map<std::string, std::vector<double>> mat;
    std::map<std::string, std::string> str;   // non-numeric scalars, quotes removed (Camera.Encoding)
};
bool parse_yaml(const std::string& text, Yaml* y, std::string* err) {
    std::istringstream in(text);
    std::string line, cur_mat;
    bool in_data = false;
    std::string data;
    auto finish_data = [&]() {
        std::vector<double> v;
        std::string tok;
        for (char& c : data) if (c == ',' || c == '[' || c == ']') c = ' ';
        std::istringstream ds(data);
        while (ds >> tok) v.push_back(std::atof(tok.c_str()));
        y->mat[cur_mat] = v;
        in_data = false; data.clear(); cur_mat.clear();
    };
    while (std::getline(in, line)) {
        if (line.rfind("%YAML", 0) == 0 || line.rfind("---", 0) == 0) continue;
        std::string s = trim(strip_comment(line));
        if (s.empty()) continue;
        if (in_data) {
            data += " " + s;
            if (s.find(']') != std::string::npos) finish_data();
            continue;
        }
        const size_t c = s.find(':');
        if (c == std::string::npos) { if (err) *err = "settings: cannot parse line '" + s + "'"; return false; }
        const std::string key = trim(s.substr(0, c)), val = trim(s.substr(c + 1));
        if (val.rfind("!!opencv-matrix", 0) == 0) { cur_mat = key; continue; }
        if (!cur_mat.empty()) {
            if (key == "data") {
                data = val; in_data = true;
                if (val.find(']') != std::string::npos) finish_data();
            }
            continue;   // rows / cols / dt
        }
        char* end = nullptr;
        const double d = std::strtod(val.c_str(), &end);
        if (end != val.c_str()) y->num[key] = d;   // non-numeric scalars (strings) are not used by the reference's hot path
        else {
            std::string v = val;
            if (v.size() >= 2 && (v.front() == '"' || v.front() == '\'') && v.back() == v.front()) v = v.substr(1, v.size() - 2);
            y->str[key] = v;
        }
    }
    return true;
}
}  // namespace

bool parse_settings(const std::string& text, Settings* out, std::string* err) {
    Yaml y;
    if (!parse_yaml(text, &y, err)) return false;
    rvio_config& c = out->cfg;
    rvio_config_euroc(&c);
    out->missing.clear();
    // (Camera.k3, Camera.Fisheye, Camera.nTimeOffset and INI.RecordOutputs are optional upstream too: absent in some of its settings files)
    auto num = [&](const char* k, double dflt) {
        auto it = y.num.find(k);
        if (it != y.num.end()) return it->second;
        const std::string ks(k);
        if (ks != "Camera.k3" && ks != "Camera.Fisheye" && ks != "Camera.nTimeOffset" && ks != "INI.RecordOutputs" && ks != "Camera.RGB") out->missing.push_back(ks);
        return dflt;
    };
    c.imu_rate = num("IMU.dps", c.imu_rate);
    c.sigma_g = num("IMU.sigma_g", c.sigma_g); c.sigma_wg = num("IMU.sigma_wg", c.sigma_wg);
    c.sigma_a = num("IMU.sigma_a", c.sigma_a); c.sigma_wa = num("IMU.sigma_wa", c.sigma_wa);
    c.gravity = num("IMU.nG", c.gravity); c.small_angle = num("IMU.nSmallAngle", c.small_angle);
    c.width = (int)num("Camera.width", c.width); c.height = (int)num("Camera.height", c.height);
    // float32, as Tracker.cc:39-62 / Updater.cc:42-44 store them
    c.fx = (float)num("Camera.fx", c.fx); c.fy = (float)num("Camera.fy", c.fy); c.cx = (float)num("Camera.cx", c.cx); c.cy = (float)num("Camera.cy", c.cy);
    c.k1 = (float)num("Camera.k1", c.k1); c.k2 = (float)num("Camera.k2", c.k2); c.p1 = (float)num("Camera.p1", c.p1); c.p2 = (float)num("Camera.p2", c.p2);
    c.k3 = (float)num("Camera.k3", c.k3);
    c.sigma_px = (float)num("Camera.sigma_px", c.sigma_px); c.sigma_py = (float)num("Camera.sigma_py", c.sigma_py);
    c.fisheye = (int)num("Camera.Fisheye", c.fisheye);
    auto m = y.mat.find("Camera.T_BC0");
    if (m == y.mat.end()) out->missing.push_back("Camera.T_BC0");
    if (m != y.mat.end()) {
        if (m->second.size() != 16) { if (err) *err = "settings: Camera.T_BC0 must hold 16 values"; return false; }
        for (int i = 0; i < 16; ++i) c.T_bc[i] = m->second[i];
    }
    c.n_features = (int)num("Tracker.nFeatures", c.n_features);
    c.max_track_len = (int)num("Tracker.nMaxTrackingLength", c.max_track_len);
    c.min_track_len = (int)num("Tracker.nMinTrackingLength", c.min_track_len);
    c.min_dist = (float)num("Tracker.nMinDist", c.min_dist); c.qual_lvl = (float)num("Tracker.nQualLvl", c.qual_lvl);
    c.block_x = (float)num("Tracker.nBlockSizeX", c.block_x); c.block_y = (float)num("Tracker.nBlockSizeY", c.block_y);
    c.enable_equalizer = (int)num("Tracker.EnableEqualizer", c.enable_equalizer);
    c.use_sampson = (int)num("Tracker.UseSampson", c.use_sampson);
    c.inlier_thr = num("Tracker.nInlierThrd", c.inlier_thr);
    c.ini_thr_angle = num("INI.nThresholdAngle", c.ini_thr_angle); c.ini_thr_displ = num("INI.nThresholdDispl", c.ini_thr_displ);
    c.ini_enable_alignment = (int)num("INI.EnableAlignment", c.ini_enable_alignment);
    out->cam_time_offset = num("Camera.nTimeOffset", 0.0);
    out->record_outputs = (int)num("INI.RecordOutputs", 0.0);
    out->is_rgb = (int)num("Camera.RGB", 0.0);
    {   // Standstill.*: optional, never reported as missing; the defaults follow the IMU densities read above
        auto opt = [&](const char* k, double dflt) { auto it = y.num.find(k); return it != y.num.end() ? it->second : dflt; };
        rvio_standstill_config& z = out->standstill;
        rvio_standstill_config_default(&c, &z);
        out->standstill_enable = (int)opt("Standstill.Enable", 0.0);
        z.sigma_a = opt("Standstill.SigmaA", z.sigma_a); z.sigma_w = opt("Standstill.SigmaW", z.sigma_w);
        z.imu_thr = opt("Standstill.ImuThr", z.imu_thr); z.disp_thr_px = opt("Standstill.DispThrPx", z.disp_thr_px);
        z.min_pairs = (int)opt("Standstill.MinPairs", z.min_pairs);
        z.sigma_v = opt("Standstill.SigmaV", z.sigma_v); z.sigma_bg = opt("Standstill.SigmaBg", z.sigma_bg);
        z.bias_rows = (int)opt("Standstill.BiasRows", z.bias_rows); z.gate = (int)opt("Standstill.Gate", z.gate);
    }
    {   // Meas.*: optional, never reported as missing
        auto it = y.num.find("Meas.Iterations");
        out->meas_iterations = it != y.num.end() ? (int)it->second : 1;
        it = y.num.find("Meas.Tolerance");
        out->meas_tolerance = it != y.num.end() ? it->second : 0.0;
    }
    out->encoding.clear();
    auto e = y.str.find("Camera.Encoding");
    if (e != y.str.end()) {
        if (encoding_format(e->second) < 0) { if (err) *err = "settings: Camera.Encoding: unknown encoding '" + e->second + "'"; return false; }
        out->encoding = e->second;
    }
    return true;
}

bool read_settings(const std::string& path, Settings* out, std::string* err) {
    std::ifstream f(path);
    if (!f) { if (err) *err = "Failed to open settings file at: " + path; return false; }   // System.cc:54-58
    std::stringstream ss; ss << f.rdbuf();
    return parse_settings(ss.str(), out, err);
}

// ------------------------------------------------------------------ InputBuffer (InputBuffer.cc:29-81)
void InputBuffer::PushImuData(const ImuData& d) {
    imu_.push_back(d);
    imu_.sort([](const ImuData& a, const ImuData& b) { return a.t < b.t; });
}
void InputBuffer::PushImageData(ImageData&& d) {
    img_.push_back(std::move(d));
    img_.sort([](const ImageData& a, const ImageData& b) { return a.t < b.t; });
}
bool InputBuffer::GetMeasurements(double off, ImageData* image, std::vector<ImuData>* imus) {
    if (imu_.empty() || img_.empty()) return false;
    if (imu_.back().t < img_.front().t + off) return false;      // not enough IMU data for this image yet
    *image = std::move(img_.front());
    img_.pop_front();
    imus->clear();
    while (!imu_.empty() && imu_.front().t <= image->t + off) { imus->push_back(imu_.front()); imu_.pop_front(); }
    return imus->size() >= 2;
}

// ------------------------------------------------------------------ System
System::System(const Settings& s, int device) : s_(s) {
    const int rc = rvio_hip_create(&s_.cfg, device, &h_);
    if (rc != RVIO_OK) {
        err_ = std::string("rvio_hip_create: ") + (h_ ? rvio_hip_last_error(h_) : "invalid configuration") + " (status " + std::to_string(rc) + ")";
        if (h_) { rvio_hip_destroy(h_); h_ = nullptr; }
        return;
    }
    if (s_.standstill_enable) {   // (a handle that is never told keeps the launches it had)
        if (rvio_hip_set_standstill(h_, &s_.standstill) != RVIO_OK) {
            err_ = std::string("Standstill.*: ") + rvio_hip_last_error(h_);
            rvio_hip_destroy(h_); h_ = nullptr;
            return;
        }
        ss_on_ = true;
    }
    if ((s_.meas_iterations != 1 || s_.meas_tolerance != 0.0) && !set_meas_iterations(s_.meas_iterations, s_.meas_tolerance)) {
        err_ = "Meas.*: " + err_;
        rvio_hip_destroy(h_); h_ = nullptr;
    }
}
bool System::set_meas_iterations(int max_iters, double tol) {
    if (!h_) { err_ = "System::set_meas_iterations without a handle"; return false; }
    if (rvio_hip_set_meas_iterations(h_, max_iters, tol) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return false; }
    return true;
}
bool System::last_meas_iter(rvio_meas_iter* out) {
    if (!h_ || rvio_hip_get_meas_iter(h_, 0, out) != RVIO_OK) { err_ = h_ ? rvio_hip_last_error(h_) : "System::last_meas_iter without a handle"; return false; }
    return true;
}
System::~System() {
    if (!ss_path_.empty()) (void)flush_standstill();
    if (f_od_ && h_) (void)flush_odometry();
    if (f_sm_ && h_) (void)flush_smoothed();
    if (f_ed_ && h_) (void)flush_edges();
    if (f_io_ && h_) (void)flush_imu_odometry();
    delete static_cast<std::ofstream*>(f_od_);
    delete static_cast<std::ofstream*>(f_sm_);
    delete static_cast<std::ofstream*>(f_ed_);
    delete static_cast<std::ofstream*>(f_io_);
    delete static_cast<std::ofstream*>(f_pose_);
    delete static_cast<std::ofstream*>(f_time_);
    delete static_cast<std::ofstream*>(f_lm_);
    delete static_cast<std::ofstream*>(f_lmc_);
    if (h_) rvio_hip_destroy(h_);
}

bool System::record_landmarks_to(const std::string& path) {
    if (!h_) return false;
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (rvio_hip_set_landmarks(h_, 1) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    delete static_cast<std::ofstream*>(f_lm_);
    f_lm_ = f;
    const int Fu = (s_.cfg.n_features + 1) / 2;
    lm_feat_.assign(Fu, 0); lm_pr_.assign((size_t)3 * Fu, 0.0); lm_pw_.assign((size_t)3 * Fu, 0.0);
    lm_last_ = -1;
    return true;
}

// behind a filtered frame: the cloud of the frame's update, if it had one (the stamp is new)
int System::write_landmarks(double t) {
    int32_t n = 0, frame = -1;
    if (rvio_hip_get_landmarks(h_, &n, &frame, lm_feat_.data(), lm_pr_.data(), lm_pw_.data()) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    if (frame < 0 || frame == lm_last_) return 0;
    lm_last_ = frame;
    auto& f = *static_cast<std::ofstream*>(f_lm_);
    f << format_landmarks(t, frame, n, lm_feat_.data(), lm_pw_.data(), lm_pr_.data());
    f.flush();
    return 0;
}

bool System::record_landmark_cov_to(const std::string& path) {
    if (!h_) return false;
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (rvio_hip_set_landmark_cov(h_, 1) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    delete static_cast<std::ofstream*>(f_lmc_);
    f_lmc_ = f;
    lmc_rec_.assign((size_t)(s_.cfg.n_features + 1) / 2, rvio_landmark_cov());
    lmc_last_ = -1;
    return true;
}

// behind a filtered frame: the records of the frame's cloud, if it had one (the stamp is new)
int System::write_landmark_cov(double t) {
    int32_t n = 0, frame = -1;
    if (rvio_hip_get_landmark_cov(h_, &n, &frame, lmc_rec_.data()) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    if (frame < 0 || frame == lmc_last_) return 0;
    lmc_last_ = frame;
    auto& f = *static_cast<std::ofstream*>(f_lmc_);
    f << format_landmark_cov(t, n, lmc_rec_.data());
    f.flush();
    return 0;
}

bool System::record_odometry_to(const std::string& path, int ring) {
    if (!h_) return false;
    if (ring < 1) { err_ = "the odometry ring holds at least one record"; return false; }
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (f_od_) (void)flush_odometry();
    if (rvio_hip_set_odometry(h_, ring) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    delete static_cast<std::ofstream*>(f_od_);
    f_od_ = f;
    od_ring_ = ring;
    od_buf_.assign((size_t)ring, rvio_odom{});
    // (records written from here on are read from here on; the handle's seq restarts with rvio_hip_initialize, which MonoVIO issues before
    // its first frame, and with a new ring)
    od_seq_ = od_read_ = ready_ ? last_seq() : 0;
    od_t_.clear();
    return true;
}

// seq of the newest record the handle has written (0: none)
long long System::last_seq() {
    rvio_odom r{};
    int64_t s = 0;
    return rvio_hip_get_odometry_all(h_, &r, &s) == RVIO_OK ? (long long)s : 0;
}

// behind a frame handed to the filter: its timestamp joins the queue; the ring is read when half of it is outstanding
int System::note_odometry(double t) {
    ++od_seq_;
    od_t_.push_back(t);
    if (od_seq_ - od_read_ >= std::max(1, od_ring_ / 2)) return flush_odometry();
    return 0;
}

int System::flush_odometry() {
    if (!f_od_ || od_seq_ == od_read_) return 0;
    int32_t n = 0;
    if (rvio_hip_get_odometry(h_, 0, od_read_ + 1, od_ring_, od_buf_.data(), &n) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    auto& f = *static_cast<std::ofstream*>(f_od_);
    for (int i = 0; i < n; ++i) {
        const rvio_odom& r = od_buf_[(size_t)i];
        // (a record the ring no longer holds was overwritten before it was read: its timestamp goes with it)
        while (od_read_ + 1 < r.seq && !od_t_.empty()) { od_t_.pop_front(); ++od_read_; }
        if (od_t_.empty()) break;
        f << format_odometry(od_t_.front(), r);
        od_t_.pop_front();
        od_read_ = r.seq;
    }
    f.flush();
    return 0;
}

bool System::record_smoothed_to(const std::string& path, int lag, int ring) {
    if (!h_) return false;
    if (ring < 1) { err_ = "the smoothed-odometry ring holds at least one record"; return false; }
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (f_sm_) (void)flush_smoothed();
    if (rvio_hip_set_smoothed_odometry(h_, ring, lag) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    delete static_cast<std::ofstream*>(f_sm_);
    f_sm_ = f;
    sm_ring_ = ring;
    sm_buf_.assign((size_t)ring, rvio_window_pose{});
    // (records written from here on are read from here on, like record_odometry_to)
    int64_t s = 0;
    sm_read_ = (ready_ && rvio_hip_get_smoothed_odometry_all(h_, sm_buf_.data(), &s) == RVIO_OK) ? (long long)s : 0;
    sm_new_ = 0;
    return true;
}

// behind a frame handed to the filter: its count and stamp join the queue; the ring is read when half of it may be outstanding
int System::note_smoothed(double t) {
    sm_t_.emplace_back(n_img_, t);
    if (++sm_new_ >= std::max(1, sm_ring_ / 2)) return flush_smoothed();
    return 0;
}

int System::flush_smoothed() {
    if (!f_sm_ || sm_new_ == 0) return 0;
    int32_t n = 0;
    if (rvio_hip_get_smoothed_odometry(h_, 0, sm_read_ + 1, sm_ring_, sm_buf_.data(), &n) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    auto& f = *static_cast<std::ofstream*>(f_sm_);
    for (int i = 0; i < n; ++i) {
        const rvio_window_pose& r = sm_buf_[(size_t)i];
        // (the stamps of frames older than the one this record describes belong to records that were never written or were overwritten)
        while (!sm_t_.empty() && sm_t_.front().first < r.img_count) sm_t_.pop_front();
        if (!sm_t_.empty() && sm_t_.front().first == r.img_count) {
            f << format_smoothed(sm_t_.front().second, r);
            sm_t_.pop_front();
        }
        sm_read_ = r.seq;
    }
    f.flush();
    sm_new_ = 0;
    return 0;
}

bool System::record_edges_to(const std::string& path, int age_new, int age_old, int ring) {
    if (!h_) return false;
    if (ring < 1) { err_ = "the edge-odometry ring holds at least one record"; return false; }
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (f_ed_) (void)flush_edges();
    if (rvio_hip_set_edge_odometry(h_, ring, age_new, age_old) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    delete static_cast<std::ofstream*>(f_ed_);
    f_ed_ = f;
    ed_ring_ = ring;
    ed_buf_.assign((size_t)ring, rvio_window_edge{});
    // (records written from here on are read from here on, like record_smoothed_to)
    int64_t s = 0;
    ed_read_ = (ready_ && rvio_hip_get_edge_odometry_all(h_, ed_buf_.data(), &s) == RVIO_OK) ? (long long)s : 0;
    ed_new_ = 0;
    return true;
}

// behind a frame handed to the filter: its count and stamp join the queue; the ring is read when half of it may be outstanding
int System::note_edges(double t) {
    ed_t_.emplace_back(n_img_, t);
    if (++ed_new_ >= std::max(1, ed_ring_ / 2)) return flush_edges();
    return 0;
}

int System::flush_edges() {
    if (!f_ed_ || ed_new_ == 0) return 0;
    int32_t n = 0;
    if (rvio_hip_get_edge_odometry(h_, 0, ed_read_ + 1, ed_ring_, ed_buf_.data(), &n) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    auto& f = *static_cast<std::ofstream*>(f_ed_);
    for (int i = 0; i < n; ++i) {
        const rvio_window_edge& r = ed_buf_[(size_t)i];
        // (frames older than this record's older end are named by no later record: the ring's ages are fixed and the counts rise)
        while (!ed_t_.empty() && ed_t_.front().first < r.img_count_old) ed_t_.pop_front();
        if (!ed_t_.empty() && ed_t_.front().first == r.img_count_old) {
            for (const auto& ct : ed_t_)
                if (ct.first == r.img_count_new) { f << format_edge(ct.second, ed_t_.front().second, r); break; }
        }
        ed_read_ = r.seq;
    }
    f.flush();
    ed_new_ = 0;
    return 0;
}

bool System::record_imu_odometry_to(const std::string& path, int ring, bool with_cov) {
    if (!h_) return false;
    if (ring < 1) { err_ = "the IMU-rate odometry ring holds at least one record"; return false; }
    auto* f = new std::ofstream(path, std::ofstream::out);
    if (!*f) { delete f; err_ = "cannot write " + path; return false; }
    if (f_io_) (void)flush_imu_odometry();
    if (rvio_hip_set_imu_odometry(h_, ring) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    if (rvio_hip_set_imu_odometry_cov(h_, with_cov ? 1 : 0) != RVIO_OK) { delete f; err_ = rvio_hip_last_error(h_); return false; }
    io_cov_ = with_cov;
    ioc_buf_.assign(with_cov ? (size_t)ring : 0, rvio_imu_cov{});
    delete static_cast<std::ofstream*>(f_io_);
    f_io_ = f;
    io_ring_ = ring;
    io_buf_.assign((size_t)ring, rvio_imu_pose{});
    // (records written from here on are read from here on: the handle's seq restarts with rvio_hip_initialize, which MonoVIO issues before its
    // first frame, and with a new ring; a ring that goes on holds its newest seq in its newest record)
    int32_t n = 0;
    io_seq_ = io_read_ = 0;
    if (ready_ && rvio_hip_get_imu_odometry(h_, 0, 1, ring, io_buf_.data(), &n) == RVIO_OK && n > 0) io_seq_ = io_read_ = io_buf_[(size_t)n - 1].seq;
    return true;
}

// behind a frame handed to the filter: its m samples are m records; the ring is read when half of it is outstanding
int System::note_imu_odometry(int m) {
    io_seq_ += m;
    if (io_seq_ - io_read_ >= std::max(1, io_ring_ / 2)) return flush_imu_odometry();
    return 0;
}

int System::flush_imu_odometry() {
    if (!f_io_ || io_seq_ == io_read_) return 0;
    int32_t n = 0;
    if (rvio_hip_get_imu_odometry(h_, 0, io_read_ + 1, io_ring_, io_buf_.data(), &n) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    auto& f = *static_cast<std::ofstream*>(f_io_);
    if (io_cov_) {   // the paired records: the same window of the same seq
        int32_t nc = 0;
        if (rvio_hip_get_imu_odometry_cov(h_, 0, io_read_ + 1, io_ring_, ioc_buf_.data(), &nc) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
        if (nc != n || (n > 0 && ioc_buf_[0].seq != io_buf_[0].seq)) { err_ = "IMU-rate odometry: the covariance ring does not hold the records of the pose ring"; return -1; }
        for (int i = 0; i < n; ++i) f << format_imu_odometry_cov(io_buf_[(size_t)i], ioc_buf_[(size_t)i]);
    } else
    for (int i = 0; i < n; ++i) f << format_imu_odometry(io_buf_[(size_t)i]);
    f.flush();
    // every outstanding sample must have come back: a ring smaller than the samples that arrive between two reads (a read follows the frame that
    // makes ring / 2 of them outstanding, so a ring below about three frames' samples, or one long batch behind dropped images) has overwritten
    // records before they were read.  The file would silently miss lines: that is an error, with the numbers that say how large the ring must be.
    const long long want = io_seq_ - io_read_;
    io_read_ = io_seq_;
    if (n != want) {
        err_ = "IMU-rate odometry: " + std::to_string(want - n) + " of " + std::to_string(want) + " records were overwritten before they were read (ring of " +
               std::to_string(io_ring_) + " samples: use a larger --imu-odometry-ring)";
        return -1;
    }
    return 0;
}

bool System::record_to(const std::string& dir, bool force) {
    if (!s_.record_outputs && !force) return true;
    auto* fp = new std::ofstream(dir + "/stamped_pose_ests.dat", std::ofstream::out);   // System.cc:86-87
    auto* ft = new std::ofstream(dir + "/time_cost.dat", std::ofstream::out);
    if (!*fp || !*ft) { delete fp; delete ft; err_ = "cannot write the record files in " + dir; return false; }
    delete static_cast<std::ofstream*>(f_pose_); delete static_cast<std::ofstream*>(f_time_);
    f_pose_ = fp; f_time_ = ft; rec_ = true;
    return true;
}

int System::device_flags() {
    if (!h_) return 0;
    rvio_frame_info fi{};
    const int rc = rvio_hip_get_frame_info(h_, &fi);
    if (rc != RVIO_OK && rc != RVIO_ERR_STATE) { err_ = rvio_hip_last_error(h_); return -1; }
    return fi.reserved[0];
}

int System::state_dim() const {
    const int n = std::min(std::max(n_img_ - 1, 0), s_.cfg.max_track_len - 1);   // (System.cc:280: the first frame augments nothing)
    return 24 + 6 * n;
}
int System::update_aux(const rvio_aux_meas& meas) {
    if (!h_ || !ready_) { err_ = "System::update_aux before the filter is initialised"; return -1; }
    if (rvio_hip_update_aux(h_, -1, &meas) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    return 0;
}
int System::velocity(const double v[3], double sigma, bool gate) {
    const int d = state_dim();
    std::vector<double> H((size_t)3 * d, 0.0);
    for (int i = 0; i < 3; ++i) H[(size_t)i * d + 15 + i] = 1.0;
    const double z[3] = {v[0], v[1], v[2]}, sg[3] = {sigma, sigma, sigma};
    rvio_aux_meas ms{};
    ms.m = 3; ms.mode = RVIO_AUX_VALUE; ms.gate = gate ? 1 : 0;
    ms.H = H.data(); ms.v = z; ms.sigma = sg;
    return update_aux(ms);
}
int System::zero_velocity(double sigma, bool gate) {
    const double z[3] = {0, 0, 0};
    return velocity(z, sigma, gate);
}

// ---- absolute fixes (rvio_hip_update_fix)
int System::update_fix(int kind, const rvio_fix& fix, bool gate) {
    if (!h_ || !ready_) { err_ = "System::update_fix before the filter is initialised"; return -1; }
    if (rvio_hip_update_fix(h_, -1, kind, gate ? 1 : 0, &fix) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    return 0;
}
rvio_fix position_fix(const double p[3], const double sigma[3], const double* lever) {
    rvio_fix f{};
    for (int i = 0; i < 3; ++i) { f.z[i] = p[i]; f.sigma[i] = sigma[i]; f.lever[i] = lever ? lever[i] : 0.0; }
    return f;
}
rvio_fix attitude_fix(const double q[4], const double sigma[3]) {
    rvio_fix f{};
    for (int i = 0; i < 4; ++i) f.z[3 + i] = q[i];
    for (int i = 0; i < 3; ++i) f.sigma[3 + i] = sigma[i];
    return f;
}
rvio_fix pose_fix(const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever) {
    rvio_fix f = position_fix(p, sigma_p, lever);
    for (int i = 0; i < 4; ++i) f.z[3 + i] = q[i];
    for (int i = 0; i < 3; ++i) f.sigma[3 + i] = sigma_q[i];
    return f;
}
rvio_fix gravity_fix(const double a[3], const double sigma[3]) { return position_fix(a, sigma, nullptr); }
int System::fix_position(const double p[3], const double sigma[3], const double* lever, bool gate) { return update_fix(RVIO_FIX_POSITION, position_fix(p, sigma, lever), gate); }
int System::fix_attitude(const double q[4], const double sigma[3], bool gate) { return update_fix(RVIO_FIX_ATTITUDE, attitude_fix(q, sigma), gate); }
int System::fix_pose(const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate) {
    return update_fix(RVIO_FIX_POSE, pose_fix(p, q, sigma_p, sigma_q, lever), gate);
}
int System::fix_gravity(const double a[3], const double sigma[3], bool gate) { return update_fix(RVIO_FIX_GRAVITY, gravity_fix(a, sigma), gate); }
// ---- past-frame fixes (rvio_hip_update_fix_past): a delayed fix fused at the frame it was taken
FixAge resolve_fix_age(const std::vector<double>& stamps, double t, bool interpolate) {
    FixAge r;
    if (stamps.empty() || !(t < stamps.front())) { r.where = FIX_AGE_NOW; return r; }      // at or past the newest composed image
    if (t < stamps.back()) { r.where = FIX_AGE_TOO_OLD; return r; }
    size_t a = 0;
    while (a + 1 < stamps.size() && !(stamps[a + 1] < t)) ++a;      // the newest a with stamps[a + 1] < t <= stamps[a] (t == the oldest stamp: the last)
    double lam = 0.0;
    if (a + 1 < stamps.size() && stamps[a] > stamps[a + 1]) lam = (stamps[a] - t) / (stamps[a] - stamps[a + 1]);
    r.where = FIX_AGE_PAST;
    if (interpolate) {
        if (lam < kFixAgeSnap) lam = 0.0;                          // (on a frame up to rounding of the stamps: that frame)
        else if (lam > 1.0 - kFixAgeSnap) { ++a; lam = 0.0; }
        r.age = (int)a; r.frac = lam;
    } else {
        r.age = (int)(lam < 0.5 ? a : a + 1); r.frac = 0.0;        // the nearest frame, a tie to the older
    }
    return r;
}
int System::update_fix_at(double t, int kind, const rvio_fix& fix, bool gate) {
    if (!h_ || !ready_) { err_ = "System::update_fix_at before the filter is initialised"; return -1; }
    const FixAge w = resolve_fix_age(std::vector<double>(stamps_.begin(), stamps_.end()), t, kind == RVIO_FIX_POSITION);
    if (w.where == FIX_AGE_NOW) return update_fix(kind, fix, gate);
    if (w.where == FIX_AGE_TOO_OLD) { ++fx_dropped_; return 0; }
    if (rvio_hip_update_fix_past(h_, -1, kind, gate ? 1 : 0, w.age, w.frac, &fix) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    return 0;
}
int System::fix_position_at(double t, const double p[3], const double sigma[3], const double* lever, bool gate) { return update_fix_at(t, RVIO_FIX_POSITION, position_fix(p, sigma, lever), gate); }
int System::fix_attitude_at(double t, const double q[4], const double sigma[3], bool gate) { return update_fix_at(t, RVIO_FIX_ATTITUDE, attitude_fix(q, sigma), gate); }
int System::fix_pose_at(double t, const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate) {
    return update_fix_at(t, RVIO_FIX_POSE, pose_fix(p, q, sigma_p, sigma_q, lever), gate);
}
// behind a composed frame: its stamp joins the window's, newest first, one per frame the clone window still reaches
void System::note_stamp(double t) {
    stamps_.push_front(t);
    const int d = state_dim();
    const size_t keep = d >= 24 ? (size_t)(d - 24) / 6 + 1 : 1;
    while (stamps_.size() > keep) stamps_.pop_back();
}
void System::queue_fixes(std::vector<FixRow> rows, bool gate, double latency) {
    std::stable_sort(rows.begin(), rows.end(), [](const FixRow& a, const FixRow& b) { return a.t < b.t; });
    fx_rows_ = std::move(rows); fx_next_ = 0; fx_gate_ = gate; fx_latency_ = latency;
}
// behind the frame stamped t: every queued fix whose stamp that frame has reached, its record handed on as parse_fixes left it (the members its
// kind does not use are 0 there, as in the typed calls' records).  With a latency (>= 0) a fix is available once the frame's stamp has reached
// its t + latency, and is fused at its own t (update_fix_at; GRAVITY has no past form: at the frame)
int System::apply_fixes(double t) {
    const bool late = fx_latency_ >= 0.0;
    for (; fx_next_ < fx_rows_.size() && fx_rows_[fx_next_].t + (late ? fx_latency_ : 0.0) <= t; ++fx_next_) {
        const FixRow& r = fx_rows_[fx_next_];
        int rc = -1;
        if (late && r.kind != RVIO_FIX_GRAVITY) rc = update_fix_at(r.t, r.kind, r.fix, fx_gate_);
        else if (r.kind < RVIO_FIX_POSITION || r.kind > RVIO_FIX_GRAVITY) err_ = "System: a queued fix of unknown kind";
        else rc = update_fix(r.kind, r.fix, fx_gate_);
        if (rc < 0) return -1;
    }
    return 0;
}
bool parse_fixes(const std::string& text, const std::string& name, std::vector<FixRow>* out, std::string* err) {
    static const char* const kNames[4] = {"position", "attitude", "pose", "gravity"};
    out->clear();
    std::istringstream in(text);
    std::string line;
    for (long ln = 1; std::getline(in, line); ++ln) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t b = line.find_first_not_of(" \t");
        if (b == std::string::npos || line[b] == '#') continue;
        auto bad = [&](const std::string& why) { *err = name + ":" + std::to_string(ln) + ": " + why + ": " + line; return false; };
        std::string flat = line;
        std::replace(flat.begin(), flat.end(), ',', ' ');
        std::istringstream ls(flat);
        std::vector<std::string> tok;
        for (std::string w; ls >> w;) tok.push_back(w);
        if (tok.size() < 2) return bad("not `t kind values... sigmas... [lever]`");
        int kind = -1;
        for (int k = 0; k < 4; ++k) if (tok[1] == kNames[k] || tok[1] == std::to_string(k)) kind = k;
        if (kind < 0) return bad("unknown kind '" + tok[1] + "' (position | attitude | pose | gravity or 0 .. 3)");
        std::vector<double> v;
        for (size_t i = 0; i < tok.size(); ++i) {
            if (i == 1) continue;
            char* end = nullptr;
            const double x = std::strtod(tok[i].c_str(), &end);
            if (end == tok[i].c_str() || *end != 0 || !std::isfinite(x)) return bad("'" + tok[i] + "' is not a finite number");
            v.push_back(x);
        }
        // v: t, then the kind's values and sigmas, then (POSITION, POSE) an optional lever
        const int nz = kind == RVIO_FIX_POSE ? 7 : (kind == RVIO_FIX_ATTITUDE ? 4 : 3), ns = kind == RVIO_FIX_POSE ? 6 : 3;
        const bool may_lever = kind == RVIO_FIX_POSITION || kind == RVIO_FIX_POSE;
        const size_t need = 1 + (size_t)nz + ns;
        if (v.size() != need && !(may_lever && v.size() == need + 3))
            return bad(std::string(kNames[kind]) + " takes " + std::to_string(nz) + " values and " + std::to_string(ns) + " sigmas" + (may_lever ? " and an optional lever of 3" : "") +
                       " behind t and the kind, the line holds " + std::to_string(v.size() - 1));
        FixRow r;
        r.t = v[0]; r.kind = kind;
        const int z0 = kind == RVIO_FIX_ATTITUDE ? 3 : 0, s0 = kind == RVIO_FIX_ATTITUDE ? 3 : 0;
        for (int i = 0; i < nz; ++i) r.fix.z[z0 + i] = v[1 + i];
        for (int i = 0; i < ns; ++i) {
            if (!(v[1 + nz + i] > 0)) return bad("a sigma is not > 0");
            r.fix.sigma[s0 + i] = v[1 + nz + i];
        }
        if (v.size() == need + 3) for (int i = 0; i < 3; ++i) r.fix.lever[i] = v[need + i];
        if (kind == RVIO_FIX_ATTITUDE || kind == RVIO_FIX_POSE) {
            const double* q = r.fix.z + 3;
            if (std::fabs(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) - 1.0) > 1e-6) return bad("the quaternion is not of unit length (1e-6)");
        }
        out->push_back(r);
    }
    return true;
}
bool read_fixes(const std::string& path, std::vector<FixRow>* out, std::string* err) {
    std::ifstream f(path);
    if (!f) { *err = "cannot read " + path; return false; }
    std::stringstream ss;
    ss << f.rdbuf();
    return parse_fixes(ss.str(), path, out, err);
}

// ---- relative-pose measurements (rvio_hip_update_rel): a delta pose between two frames of the window
RelSpan resolve_rel_span(const std::vector<double>& stamps, double t_new, double t_old) {
    RelSpan r;
    if (stamps.empty()) return r;
    const FixAge a = resolve_fix_age(stamps, t_new, false), b = resolve_fix_age(stamps, t_old, false);
    if (a.where == FIX_AGE_TOO_OLD || b.where == FIX_AGE_TOO_OLD) return r;                  // the older stamp (or both) has left the window
    r.age_new = a.where == FIX_AGE_NOW ? 0 : a.age;                                          // at or past the newest composed image: that image
    r.age_old = b.where == FIX_AGE_NOW ? 0 : b.age;
    r.ok = r.age_new < r.age_old;                                                            // (one frame has no delta)
    return r;
}
int System::update_rel_at(double t_new, double t_old, int kind, const rvio_fix& meas, bool gate) {
    if (!h_ || !ready_) { err_ = "System::update_rel_at before the filter is initialised"; return -1; }
    if (!(t_old < t_new)) { err_ = "System::update_rel_at: t_old is not before t_new"; return -1; }
    const RelSpan w = resolve_rel_span(std::vector<double>(stamps_.begin(), stamps_.end()), t_new, t_old);
    if (!w.ok) { ++rl_dropped_; return 0; }
    if (rvio_hip_update_rel(h_, -1, kind, gate ? 1 : 0, w.age_new, w.age_old, &meas) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    return 0;
}
int System::rel_position_at(double t_new, double t_old, const double d[3], const double sigma[3], const double* lever, bool gate) {
    return update_rel_at(t_new, t_old, RVIO_REL_POSITION, position_fix(d, sigma, lever), gate);
}
int System::rel_attitude_at(double t_new, double t_old, const double q[4], const double sigma[3], bool gate) {
    return update_rel_at(t_new, t_old, RVIO_REL_ATTITUDE, attitude_fix(q, sigma), gate);
}
int System::rel_pose_at(double t_new, double t_old, const double d[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate) {
    return update_rel_at(t_new, t_old, RVIO_REL_POSE, pose_fix(d, q, sigma_p, sigma_q, lever), gate);
}
void System::queue_rels(std::vector<RelRow> rows, bool gate) {
    std::stable_sort(rows.begin(), rows.end(), [](const RelRow& a, const RelRow& b) { return a.t_new < b.t_new; });
    rl_rows_ = std::move(rows); rl_next_ = 0; rl_gate_ = gate;
}
// behind the frame stamped t: every queued measurement whose newer stamp that frame has reached
int System::apply_rels(double t) {
    for (; rl_next_ < rl_rows_.size() && rl_rows_[rl_next_].t_new <= t; ++rl_next_) {
        const RelRow& r = rl_rows_[rl_next_];
        if (update_rel_at(r.t_new, r.t_old, r.kind, r.meas, rl_gate_) < 0) return -1;
    }
    return 0;
}
bool parse_rels(const std::string& text, const std::string& name, std::vector<RelRow>* out, std::string* err) {
    static const char* const kNames[3] = {"position", "attitude", "pose"};
    out->clear();
    std::istringstream in(text);
    std::string line;
    for (long ln = 1; std::getline(in, line); ++ln) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t b = line.find_first_not_of(" \t");
        if (b == std::string::npos || line[b] == '#') continue;
        auto bad = [&](const std::string& why) { *err = name + ":" + std::to_string(ln) + ": " + why + ": " + line; return false; };
        std::string flat = line;
        std::replace(flat.begin(), flat.end(), ',', ' ');
        std::istringstream ls(flat);
        std::vector<std::string> tok;
        for (std::string w; ls >> w;) tok.push_back(w);
        if (tok.size() < 3) return bad("not `t_new t_old kind values... sigmas... [lever]`");
        int k = -1;
        for (int i = 0; i < 3; ++i) if (tok[2] == kNames[i] || tok[2] == std::to_string(RVIO_REL_POSITION + i)) k = i;
        if (k < 0) return bad("unknown kind '" + tok[2] + "' (position | attitude | pose or 16 .. 18)");
        std::vector<double> v;
        for (size_t i = 0; i < tok.size(); ++i) {
            if (i == 2) continue;
            char* end = nullptr;
            const double x = std::strtod(tok[i].c_str(), &end);
            if (end == tok[i].c_str() || *end != 0 || !std::isfinite(x)) return bad("'" + tok[i] + "' is not a finite number");
            v.push_back(x);
        }
        // v: t_new, t_old, then the kind's values and sigmas, then (position, pose) an optional lever
        const int nz = k == 2 ? 7 : (k == 1 ? 4 : 3), ns = k == 2 ? 6 : 3;
        const bool may_lever = k != 1;
        const size_t need = 2 + (size_t)nz + ns;
        if (v.size() != need && !(may_lever && v.size() == need + 3))
            return bad(std::string(kNames[k]) + " takes " + std::to_string(nz) + " values and " + std::to_string(ns) + " sigmas" + (may_lever ? " and an optional lever of 3" : "") +
                       " behind the two stamps and the kind, the line holds " + std::to_string(v.size() - 2));
        RelRow r;
        r.t_new = v[0]; r.t_old = v[1]; r.kind = RVIO_REL_POSITION + k;
        if (!(r.t_old < r.t_new)) return bad("t_old is not before t_new");
        const int z0 = k == 1 ? 3 : 0;
        for (int i = 0; i < nz; ++i) r.meas.z[z0 + i] = v[2 + i];
        for (int i = 0; i < ns; ++i) {
            if (!(v[2 + nz + i] > 0)) return bad("a sigma is not > 0");
            r.meas.sigma[z0 + i] = v[2 + nz + i];
        }
        if (v.size() == need + 3) for (int i = 0; i < 3; ++i) r.meas.lever[i] = v[need + i];
        if (k != 0) {
            const double* q = r.meas.z + 3;
            if (std::fabs(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) - 1.0) > 1e-6) return bad("the quaternion is not of unit length (1e-6)");
        }
        out->push_back(r);
    }
    return true;
}
bool read_rels(const std::string& path, std::vector<RelRow>* out, std::string* err) {
    std::ifstream f(path);
    if (!f) { *err = "cannot read " + path; return false; }
    std::stringstream ss;
    ss << f.rdbuf();
    return parse_rels(ss.str(), path, out, err);
}

// ---- map landmarks (rvio_hip_update_map): pixel observations of known world points at the image they were matched in
MapAge resolve_map_age(const std::vector<double>& stamps, double t) {
    MapAge r;
    if (stamps.empty()) return r;
    const FixAge a = resolve_fix_age(stamps, t, false);
    if (a.where == FIX_AGE_TOO_OLD) return r;
    r.ok = true;
    r.age = a.where == FIX_AGE_NOW ? 0 : a.age;
    return r;
}
std::vector<std::pair<int, int>> map_calls(int n) {
    std::vector<std::pair<int, int>> out;
    for (int first = 0; first < n; first += RVIO_MAP_MAX_POINTS) out.emplace_back(first, std::min(RVIO_MAP_MAX_POINTS, n - first));
    return out;
}
int System::map_points_at(double t, const rvio_map_obs* pts, int n, int units, bool gate_each) {
    if (!h_ || !ready_) { err_ = "System::map_points_at before the filter is initialised"; return -1; }
    if (!pts || n < 1) { err_ = "System::map_points_at: no observations"; return -1; }
    const MapAge w = resolve_map_age(std::vector<double>(stamps_.begin(), stamps_.end()), t);
    if (!w.ok) { mp_skipped_.push_back(t); return 0; }
    for (const std::pair<int, int>& c : map_calls(n))
        if (rvio_hip_update_map(h_, -1, units, 0, gate_each ? 1 : 0, w.age, c.second, pts + c.first) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    return 0;
}
void System::queue_map(std::vector<MapRow> rows, int units, double latency, bool gate_each) {
    std::stable_sort(rows.begin(), rows.end(), [](const MapRow& a, const MapRow& b) { return a.t < b.t; });
    mp_rows_ = std::move(rows); mp_next_ = 0; mp_units_ = units; mp_latency_ = latency > 0 ? latency : 0.0; mp_gate_ = gate_each; mp_groups_ = 0; mp_skipped_.clear();
}
// behind the frame stamped t: every queued group whose stamp + latency that frame has reached, fused at the group's own stamp
int System::apply_map(double t) {
    while (mp_next_ < mp_rows_.size() && mp_rows_[mp_next_].t + mp_latency_ <= t) {
        const double tg = mp_rows_[mp_next_].t;
        std::vector<rvio_map_obs> pts;
        for (; mp_next_ < mp_rows_.size() && mp_rows_[mp_next_].t == tg; ++mp_next_) pts.push_back(mp_rows_[mp_next_].obs);
        ++mp_groups_;
        if (map_points_at(tg, pts.data(), (int)pts.size(), mp_units_, mp_gate_) < 0) return -1;
    }
    return 0;
}
bool parse_map(const std::string& text, const std::string& name, std::vector<MapRow>* out, std::string* err) {
    out->clear();
    std::istringstream in(text);
    std::string line;
    for (long ln = 1; std::getline(in, line); ++ln) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t b = line.find_first_not_of(" \t");
        if (b == std::string::npos || line[b] == '#') continue;
        auto bad = [&](const std::string& why) { *err = name + ":" + std::to_string(ln) + ": " + why + ": " + line; return false; };
        std::string flat = line;
        std::replace(flat.begin(), flat.end(), ',', ' ');
        std::istringstream ls(flat);
        std::vector<double> v;
        for (std::string w; ls >> w;) {
            char* end = nullptr;
            const double x = std::strtod(w.c_str(), &end);
            if (end == w.c_str() || *end != 0 || !std::isfinite(x)) return bad("'" + w + "' is not a finite number");
            v.push_back(x);
        }
        if (v.size() != 7) return bad("not `t x y z u v sigma`, the line holds " + std::to_string(v.size()) + " fields");
        if (!(v[6] > 0)) return bad("sigma is not > 0");
        MapRow r;
        r.t = v[0];
        for (int i = 0; i < 3; ++i) r.obs.p_w[i] = v[1 + i];
        r.obs.uv[0] = v[4]; r.obs.uv[1] = v[5]; r.obs.sigma = v[6];
        out->push_back(r);
    }
    return true;
}
bool read_map(const std::string& path, std::vector<MapRow>* out, std::string* err) {
    std::ifstream f(path);
    if (!f) { *err = "cannot read " + path; return false; }
    std::stringstream ss;
    ss << f.rdbuf();
    return parse_map(ss.str(), path, out, err);
}

// behind a frame: the decision and, where the platform stands still, the zero-velocity update — on the device, nothing waited for unless the
// records are asked for
int System::standstill(double t, const rvio_imu* imu, int m) {
    if (m < 1) return 0;
    if (rvio_hip_standstill(h_, imu, m, 1) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
    if (!ss_path_.empty()) {
        rvio_standstill r;
        if (rvio_hip_get_standstill(h_, 0, &r) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
        ss_recs_.emplace_back(t, r);
    }
    return 0;
}
bool System::record_standstill_to(const std::string& path) {
    if (!h_) return false;
    if (!ss_on_) { err_ = "--standstill needs Standstill.Enable: 1 in the settings"; return false; }
    std::ofstream f(path, std::ofstream::out);   // (created now: an unwritable path fails here, not after the replay)
    if (!f) { err_ = "cannot write " + path; return false; }
    ss_path_ = path;
    ss_recs_.clear();
    return true;
}
int System::flush_standstill() {
    if (ss_path_.empty()) return 0;
    std::ofstream f(ss_path_, std::ofstream::out);
    if (!f) { err_ = "cannot write " + ss_path_; return -1; }
    for (const auto& tr : ss_recs_) f << format_standstill(tr.first, tr.second);
    f.flush();
    return f ? 0 : -1;
}
std::string format_standstill(double t, const rvio_standstill& r) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%.19g %.19g %.19g %d %d %.19g\n", t, r.T, r.disparity, (int)r.n_pairs, (int)r.flags, r.gamma);
    return buf;
}

int System::MonoVIO(PoseLine* pose) {
    ImageData image;
    std::vector<ImuData> imus;
    if (!buf_.GetMeasurements(s_.cam_time_offset, &image, &imus)) return 0;
    size_t first = 0;                                  // samples before `first` were consumed by the start-up average
    if (!ready_) {                                     // System.cc:185-250
        if (!moving_) {
            double ang[3] = {0, 0, 0}, vel[3] = {0, 0, 0}, displ[3] = {0, 0, 0};
            for (const ImuData& d : imus) {
                const double an = std::sqrt(d.a[0] * d.a[0] + d.a[1] * d.a[1] + d.a[2] * d.a[2]);
                for (int i = 0; i < 3; ++i) {
                    const double a = d.a[i] - s_.cfg.gravity * d.a[i] / an;
                    ang[i] += d.dt * d.w[i];
                    vel[i] += d.dt * a;
                    displ[i] += d.dt * vel[i] + .5 * d.dt * d.dt * a;
                }
            }
            const double na = std::sqrt(ang[0] * ang[0] + ang[1] * ang[1] + ang[2] * ang[2]);
            const double nd = std::sqrt(displ[0] * displ[0] + displ[1] * displ[1] + displ[2] * displ[2]);
            if (na > s_.cfg.ini_thr_angle || nd > s_.cfg.ini_thr_displ) moving_ = true;
        }
        while (first < imus.size()) {
            if (!moving_) {
                for (int i = 0; i < 3; ++i) { wm_[i] += imus[first].w[i]; am_[i] += imus[first].a[i]; }
                ++first; ++n_imu_;
            } else {
                if (n_imu_ == 0) {
                    for (int i = 0; i < 3; ++i) { wm_[i] = imus[first].w[i]; am_[i] = imus[first].a[i]; }
                    n_imu_ = 1;
                } else
                    for (int i = 0; i < 3; ++i) { wm_[i] /= n_imu_; am_[i] /= n_imu_; }
                if (rvio_hip_initialize(h_, wm_, am_, n_imu_) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
                ready_ = true;
                stamps_.clear();
                // (rvio_hip_initialize restarts the handle's frame count and empties the smoothed ring: the stamps, which are matched to records by
                // that count — n_img_ mirrors it, both count the frames handed to the filter since this point —, start over with it)
                sm_t_.clear(); sm_read_ = 0; sm_new_ = 0;
                ed_t_.clear(); ed_read_ = 0; ed_new_ = 0;   // (the edge ring likewise)
                break;
            }
        }
        if (!ready_) return 0;
    }
    ++n_img_;
    static_assert(sizeof(ImuData) == sizeof(rvio_imu), "ImuData mirrors rvio_imu");
    const rvio_imu* pi = reinterpret_cast<const rvio_imu*>(imus.data() + first);
    const int m = (int)(imus.size() - first);
    // (any number of samples: a gap of a few dropped images is integrated in one go as upstream does, PreIntegrator.cc:96-97; beyond
    // RVIO_HIP_MAX_IMU = 192 the library grows its staging once)
    if (image.width != s_.cfg.width || image.height != s_.cfg.height) { err_ = "image size does not match Camera.width/height"; return -1; }
    // "Convert to gray scale" (Tracker.cc:182-196) runs on the device: the handle is told what a pixel is — once, and again only when the channel
    // count of the stream changes — and takes the interleaved bytes as they are (to_gray below is the host form of the same arithmetic)
    // (... and what cv_bridge converts in front of Tracker::track, rvio_mono.cc:64: 16-bit samples and Bayer mosaics go over unconverted too)
    const int fmt = image_format(image, s_, &err_);
    if (fmt < 0) return -1;
    if (fmt != pix_fmt_) {
        if (rvio_hip_set_image_format(h_, fmt) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
        pix_fmt_ = fmt;
    }
    const int row_bytes = image.width * image.channels * (image.bits / 8);
    if (image.px.size() < (size_t)row_bytes * image.height) { err_ = "image holds fewer bytes than width x height x channels"; return -1; }
    // the timed body of MonoVIO (System.cc:253-367): track -> propagate -> update -> augment -> compose
    if (!rec_) {
        if (rvio_hip_frame(h_, image.px.data(), row_bytes, pi, m, nullptr, 0) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
        note_stamp(image.t);
        if (ss_on_ && standstill(image.t, pi, m) < 0) return -1;   // (ahead of the pose read-back: the pose line is the updated state's)
        if (fx_next_ < fx_rows_.size() && apply_fixes(image.t) < 0) return -1;   // (likewise)
        if (rl_next_ < rl_rows_.size() && apply_rels(image.t) < 0) return -1;    // (likewise)
        if (mp_next_ < mp_rows_.size() && apply_map(image.t) < 0) return -1;     // (likewise)
        if (pose) {
            pose->t = image.t;
            if (rvio_hip_get_pose(h_, pose->p, pose->q) != RVIO_OK) { err_ = rvio_hip_last_error(h_); return -1; }
        }
        if (f_lm_ && write_landmarks(image.t) < 0) return -1;
    if (f_lmc_ && write_landmark_cov(image.t) < 0) return -1;
        if (f_od_ && note_odometry(image.t) < 0) return -1;
        if (f_sm_ && note_smoothed(image.t) < 0) return -1;
        if (f_ed_ && note_edges(image.t) < 0) return -1;
        if (f_io_ && note_imu_odometry(m) < 0) return -1;
        return 1;
    }
    // INI.RecordOutputs: the same body stage by stage with the host waiting behind each, t1 / t2 / t3 taken where upstream takes them
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto fail = [&] { err_ = rvio_hip_last_error(h_); return -1; };
    const double t1 = now();
    if (rvio_hip_track(h_, image.px.data(), row_bytes, pi, m, nullptr, 0) != RVIO_OK || rvio_hip_sync(h_) != RVIO_OK) return fail();   // System.cc:258
    const double t2 = now();
    int do_update = 0, do_augment = 0;
    if (rvio_hip_frame_plan(h_, &do_update, &do_augment) != RVIO_OK) return fail();
    if (rvio_hip_propagate(h_, pi, m) != RVIO_OK) return fail();                          // System.cc:263
    if (do_update && rvio_hip_update_tracked(h_) != RVIO_OK) return fail();               // System.cc:266-268
    if (rvio_hip_augment_compose(h_, do_augment) != RVIO_OK) return fail();               // System.cc:279-365
    note_stamp(image.t);
    if (ss_on_ && standstill(image.t, pi, m) < 0) return -1;
    if (fx_next_ < fx_rows_.size() && apply_fixes(image.t) < 0) return -1;
    if (rl_next_ < rl_rows_.size() && apply_rels(image.t) < 0) return -1;
    if (mp_next_ < mp_rows_.size() && apply_map(image.t) < 0) return -1;
    PoseLine pl;
    pl.t = image.t;
    if (rvio_hip_get_pose(h_, pl.p, pl.q) != RVIO_OK) return fail();                      // (waits for the filter stream)
    const double t3 = now();
    auto& fp = *static_cast<std::ofstream*>(f_pose_);
    auto& ft = *static_cast<std::ofstream*>(f_time_);
    fp << format_pose(pl); fp.flush();
    ft << format_time_cost(n_img_, t2 - t1, t3 - t2); ft.flush();
    if (f_lm_ && write_landmarks(image.t) < 0) return -1;
    if (f_lmc_ && write_landmark_cov(image.t) < 0) return -1;
    if (f_od_ && note_odometry(image.t) < 0) return -1;
    if (f_sm_ && note_smoothed(image.t) < 0) return -1;
    if (f_ed_ && note_edges(image.t) < 0) return -1;
    if (f_io_ && note_imu_odometry(m) < 0) return -1;
    if (pose) *pose = pl;
    return 1;
}

std::string format_time_cost(int n_img, double track_ms, double filter_ms) {   // nImageCountAfterInit, 1e3 (t2-t1), 1e3 (t3-t2); setprecision(19)
    char buf[160];
    std::snprintf(buf, sizeof buf, "%d %.19g %.19g\n", n_img, track_ms, filter_ms);
    return buf;
}

std::string format_pose(const PoseLine& p) {
    char buf[512];
    std::snprintf(buf, sizeof buf, "%.19g %.19g %.19g %.19g %.19g %.19g %.19g %.19g\n", p.t, p.p[0], p.p[1], p.p[2], p.q[0], p.q[1], p.q[2], p.q[3]);
    return buf;
}

std::string format_odometry(double t, const rvio_odom& r) {
    char buf[64];
    std::string out;
    auto add = [&](double v) { std::snprintf(buf, sizeof buf, " %.19g", v); out += buf; };
    std::snprintf(buf, sizeof buf, "%.19g %lld", t, (long long)r.seq);
    out = buf;
    for (double v : r.p) add(v);
    for (double v : r.q) add(v);
    for (double v : r.v) add(v);
    for (double v : r.pose_cov) add(v);
    out += "\n";
    return out;
}

std::string format_smoothed(double t, const rvio_window_pose& r) {
    rvio_odom o{};
    o.seq = r.seq;
    std::copy(r.p, r.p + 3, o.p); std::copy(r.q, r.q + 4, o.q); std::copy(r.pose_cov, r.pose_cov + 36, o.pose_cov);
    return format_odometry(t, o);
}

std::string format_edge(double t_new, double t_old, const rvio_window_edge& r) {
    char buf[64];
    std::string out;
    auto put = [&](double v, const char* sep) { std::snprintf(buf, sizeof buf, "%.19g%s", v, sep); out += buf; };
    put(t_new, " "); put(t_old, " ");
    for (int i = 0; i < 3; ++i) put(r.p[i], " ");
    for (int i = 0; i < 4; ++i) put(r.q[i], " ");
    for (int i = 0; i < 36; ++i) put(r.cov[i], i == 35 ? "\n" : " ");
    return out;
}

std::string format_imu_odometry(const rvio_imu_pose& r) {
    char buf[64];
    std::string out;
    auto add = [&](double v) { std::snprintf(buf, sizeof buf, " %.19g", v); out += buf; };
    std::snprintf(buf, sizeof buf, "%.19g", r.t);
    out = buf;
    for (double v : r.p) add(v);
    for (double v : r.q) add(v);
    for (double v : r.v) add(v);
    out += "\n";
    return out;
}

std::string format_imu_odometry_cov(const rvio_imu_pose& r, const rvio_imu_cov& c) {
    char buf[64];
    std::string out = format_imu_odometry(r);
    out.pop_back();   // (its newline)
    auto add = [&](double v) { std::snprintf(buf, sizeof buf, " %.19g", v); out += buf; };
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) add(c.pose_cov[6 * i + j]);
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) add(c.vel_cov[3 * i + j]);
    out += "\n";
    return out;
}

std::string format_landmarks(double t, int frame, int n, const int32_t* feat, const double* p_world, const double* p_r) {
    std::string out;
    char buf[512];
    for (int i = 0; i < n; ++i) {
        const double *w = p_world + 3 * i, *r = p_r + 3 * i;
        std::snprintf(buf, sizeof buf, "%.19g %d %d %.19g %.19g %.19g %.19g %.19g %.19g\n", t, frame, (int)feat[i], w[0], w[1], w[2], r[0], r[1], r[2]);
        out += buf;
    }
    return out;
}

std::string format_landmark_cov(double t, int n, const rvio_landmark_cov* rec) {
    std::string out;
    char buf[64];
    for (int i = 0; i < n; ++i) {
        const rvio_landmark_cov& r = rec[i];
        std::snprintf(buf, sizeof buf, "%.19g %d %d %d", t, (int)r.feat, (int)r.n_obs, (int)r.status);
        out += buf;
        auto add = [&](double v) { std::snprintf(buf, sizeof buf, " %.19g", v); out += buf; };
        for (int k = 0; k < 3; ++k) add(r.p_w[k]);
        for (int a = 0; a < 3; ++a) for (int b = a; b < 3; ++b) add(r.cov_w[3 * a + b]);
        for (int k = 0; k < 3; ++k) add(r.p_r[k]);
        for (int a = 0; a < 3; ++a) for (int b = a; b < 3; ++b) add(r.cov_r[3 * a + b]);
        add(r.rho); add(r.rho_sigma);
        out += "\n";
    }
    return out;
}

// ------------------------------------------------------------------ images
int encoding_format(const std::string& name) {
    static const struct { const char* n; int f; } table[] = {
        {"mono8", RVIO_PIX_MONO8}, {"rgb8", RVIO_PIX_RGB8}, {"bgr8", RVIO_PIX_BGR8}, {"rgba8", RVIO_PIX_RGBA8}, {"bgra8", RVIO_PIX_BGRA8},
        {"mono16", RVIO_PIX_MONO16}, {"rgb16", RVIO_PIX_RGB16}, {"bgr16", RVIO_PIX_BGR16}, {"rgba16", RVIO_PIX_RGBA16}, {"bgra16", RVIO_PIX_BGRA16},
        {"bayer_rggb8", RVIO_PIX_BAYER_RGGB8}, {"bayer_bggr8", RVIO_PIX_BAYER_BGGR8}, {"bayer_gbrg8", RVIO_PIX_BAYER_GBRG8}, {"bayer_grbg8", RVIO_PIX_BAYER_GRBG8},
        {"bayer_rggb16", RVIO_PIX_BAYER_RGGB16}, {"bayer_bggr16", RVIO_PIX_BAYER_BGGR16}, {"bayer_gbrg16", RVIO_PIX_BAYER_GBRG16},
        {"bayer_grbg16", RVIO_PIX_BAYER_GRBG16}};
    for (const auto& e : table) if (name == e.n) return e.f;
    return -1;
}
namespace {
// rvio_pixel_format: bit 4 = 16-bit samples, bit 5 = a mosaic, else 0 mono, 1 / 2 three samples, 3 / 4 four
int fmt_bits(int f) { return (f & 16) ? 16 : 8; }
bool fmt_bayer(int f) { return (f & 32) != 0; }
int fmt_samples(int f) { return fmt_bayer(f) || (f & 15) == 0 ? 1 : (f & 15) <= 2 ? 3 : 4; }
bool fmt_bgr(int f) { return !fmt_bayer(f) && ((f & 15) == 2 || (f & 15) == 4); }
}  // namespace

int image_format(const ImageData& im, const Settings& s, std::string* err) {
    if ((im.channels != 1 && im.channels != 3 && im.channels != 4) || (im.bits != 8 && im.bits != 16)) {
        if (err) *err = "images of 1, 3 or 4 channels and 8 or 16 bits are supported";
        return -1;
    }
    if (s.encoding.empty()) {
        const int k = im.channels == 1 ? RVIO_PIX_MONO8 : im.channels == 3 ? (s.is_rgb ? RVIO_PIX_RGB8 : RVIO_PIX_BGR8) : (s.is_rgb ? RVIO_PIX_RGBA8 : RVIO_PIX_BGRA8);
        return im.bits == 16 ? (k | 16) : k;
    }
    const int f = encoding_format(s.encoding);
    if (f < 0 || fmt_samples(f) != im.channels || fmt_bits(f) != im.bits) {
        if (err) *err = "Camera.Encoding: " + s.encoding + " contradicts the image (" + std::to_string(im.channels) + " channel(s) of " + std::to_string(im.bits) + " bits)";
        return -1;
    }
    return f;
}

bool to_gray(ImageData* im, int format, std::string* err) {
    if (format < 0 || fmt_samples(format) != im->channels || fmt_bits(format) != im->bits) { if (err) *err = "the image format does not fit the image's channels and bit depth"; return false; }
    const size_t n = (size_t)im->width * im->height;
    if (im->px.size() < n * im->channels * (im->bits / 8)) { if (err) *err = "image holds fewer bytes than width x height x channels"; return false; }
    if (fmt_bayer(format)) {
        if (im->width < 3 || im->height < 3) { if (err) *err = "a Bayer mosaic needs at least 3 x 3 pixels"; return false; }
        std::vector<uint8_t> g(n);
        const BayerP b = bayer_pattern(format & 3);
        for (int y = 0; y < im->height; ++y)
            for (int x = 0; x < im->width; ++x)
                g[(size_t)y * im->width + x] = (uint8_t)(im->bits == 16 ? bayer_at<uint16_t>((const uint16_t*)im->px.data(), im->width, im->width, im->height, x, y, b)
                                                                         : bayer_at<uint8_t>(im->px.data(), im->width, im->width, im->height, x, y, b));
        im->px.swap(g);
    } else if (im->bits == 16) {
        const GrayW w = gray_weights(fmt_bgr(format) ? 1 : 0);
        const int c = im->channels;
        const uint16_t* p = (const uint16_t*)im->px.data();   // (in place: pixel i is read before byte i is written)
        for (size_t i = 0; i < n; ++i) im->px[i] = (uint8_t)(c == 1 ? raw_depth8(p[i]) : raw16_px(p[i * c], p[i * c + 1], p[i * c + 2], w));
        im->px.resize(n);
    } else to_gray(im, !fmt_bgr(format));
    im->channels = 1; im->bits = 8;
    return true;
}

void to_gray(ImageData* im, bool is_rgb) {
    const int c = im->channels;
    if (im->bits == 16) { to_gray(im, (c == 1 ? RVIO_PIX_MONO16 : c == 3 ? (is_rgb ? RVIO_PIX_RGB16 : RVIO_PIX_BGR16) : (is_rgb ? RVIO_PIX_RGBA16 : RVIO_PIX_BGRA16)), nullptr); return; }
    if (c != 3 && c != 4) return;
    const size_t n = (size_t)im->width * im->height;
    const int ir = is_rgb ? 0 : 2, ib = is_rgb ? 2 : 0;          // byte position of R and B inside a pixel
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* p = &im->px[i * c];
        im->px[i] = (uint8_t)((p[ir] * 4899 + p[1] * 9617 + p[ib] * 1868 + (1 << 13)) >> 14);   // cv::cvtColor 8u: R2Y, G2Y, B2Y, yuv_shift = 14
    }
    im->px.resize(n);
    im->channels = 1;
}

bool decode_png_gray8(const uint8_t* d, size_t n, ImageData* out, std::string* err) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (n < 8 || std::memcmp(d, sig, 8) != 0) { if (err) *err = "not a PNG"; return false; }
    auto be32 = [&](size_t o) { return ((uint32_t)d[o] << 24) | ((uint32_t)d[o + 1] << 16) | ((uint32_t)d[o + 2] << 8) | d[o + 3]; };
    size_t o = 8;
    uint32_t w = 0, h = 0, bpp = 1, depth = 8;
    std::vector<uint8_t> z;
    bool have_hdr = false;
    while (o + 12 <= n) {
        const uint32_t len = be32(o);
        const char* type = (const char*)d + o + 4;
        if (o + 12 + len > n) break;
        const uint8_t* p = d + o + 8;
        if (!std::memcmp(type, "IHDR", 4)) {
            w = be32(o + 8); h = be32(o + 12);
            if ((p[8] != 8 && p[8] != 16) || (p[9] != 0 && p[9] != 2 && p[9] != 6) || p[12] != 0) { if (err) *err = "PNG: only 8- and 16-bit gray / RGB / RGBA, non-interlaced images are supported"; return false; }
            depth = p[8];
            bpp = (p[9] == 0 ? 1 : (p[9] == 2 ? 3 : 4)) * (depth / 8);   // bytes per pixel: the distance the filters look back
            have_hdr = true;
        } else if (!std::memcmp(type, "IDAT", 4)) z.insert(z.end(), p, p + len);
        else if (!std::memcmp(type, "IEND", 4)) break;
        o += 12 + len;
    }
    if (!have_hdr || w == 0 || h == 0) { if (err) *err = "PNG: no header"; return false; }
    const size_t rowb = (size_t)w * bpp;
    std::vector<uint8_t> raw((rowb + 1) * h);
    uLongf rl = (uLongf)raw.size();
    if (uncompress(raw.data(), &rl, z.data(), (uLong)z.size()) != Z_OK || rl != raw.size()) { if (err) *err = "PNG: inflate failed"; return false; }
    out->width = (int)w; out->height = (int)h; out->channels = (int)(bpp / (depth / 8)); out->bits = (int)depth; out->px.assign(rowb * h, 0);
    for (uint32_t y = 0; y < h; ++y) {                 // un-filter
        const uint8_t ft = raw[(size_t)y * (rowb + 1)];
        const uint8_t* s = &raw[(size_t)y * (rowb + 1) + 1];
        uint8_t* r = &out->px[(size_t)y * rowb];
        const uint8_t* up = y ? r - rowb : nullptr;
        for (size_t x = 0; x < rowb; ++x) {
            const int a = x >= bpp ? r[x - bpp] : 0, b = up ? up[x] : 0, c = (x >= bpp && up) ? up[x - bpp] : 0;
            int pred = 0;
            switch (ft) {
                case 0: pred = 0; break;
                case 1: pred = a; break;
                case 2: pred = b; break;
                case 3: pred = (a + b) >> 1; break;
                case 4: { const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
                default: if (err) *err = "PNG: bad filter type"; return false;
            }
            r[x] = (uint8_t)(s[x] + pred);
        }
    }
    if (depth == 16) {   // big-endian samples -> host order
        uint16_t* q = (uint16_t*)out->px.data();
        for (size_t i = 0; i < out->px.size() / 2; ++i) q[i] = (uint16_t)((out->px[2 * i] << 8) | out->px[2 * i + 1]);
    }
    return true;
}

bool read_image(const std::string& path, ImageData* out, std::string* err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { if (err) *err = "cannot open " + path; return false; }
    std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (buf.size() >= 2 && buf[0] == 'P' && (buf[1] == '5' || buf[1] == '6')) {   // binary PGM / PPM: P5|P6 <w> <h> <maxval> <single whitespace> data
        const size_t ch = buf[1] == '6' ? 3 : 1;
        size_t o = 2;
        long v[3];
        for (int k = 0; k < 3; ++k) {
            while (o < buf.size() && (std::isspace(buf[o]) || buf[o] == '#')) { if (buf[o] == '#') while (o < buf.size() && buf[o] != '\n') ++o; else ++o; }
            long x = 0; bool any = false;
            while (o < buf.size() && std::isdigit(buf[o])) { x = 10 * x + (buf[o] - '0'); ++o; any = true; }
            if (!any) { if (err) *err = "PGM: bad header in " + path; return false; }
            v[k] = x;
        }
        ++o;
        const size_t sb = v[2] > 255 ? 2 : 1;   // Netpbm: two bytes per sample, most significant first, from maxval 256 on
        if (v[2] < 255 || v[2] > 65535 || o + (size_t)v[0] * v[1] * ch * sb > buf.size()) { if (err) *err = "PGM/PPM: only maxval 255 (8 bits) and 256 .. 65535 (16 bits) are supported (" + path + ")"; return false; }
        out->width = (int)v[0]; out->height = (int)v[1]; out->channels = (int)ch; out->bits = (int)(8 * sb);
        out->px.assign(buf.begin() + o, buf.begin() + o + (size_t)v[0] * v[1] * ch * sb);
        if (sb == 2) {
            uint16_t* q = (uint16_t*)out->px.data();
            for (size_t i = 0; i < out->px.size() / 2; ++i) q[i] = (uint16_t)((out->px[2 * i] << 8) | out->px[2 * i + 1]);
        }
        return true;
    }
    std::string e;
    if (!decode_png_gray8(buf.data(), buf.size(), out, &e)) { if (err) *err = e + " (" + path + ")"; return false; }
    return true;
}

// ------------------------------------------------------------------ EuRoC ASL folder
bool read_asl(const std::string& root, AslDataset* out, std::string* err) {
    auto open = [&](const std::string& rel, std::ifstream& f) {
        f.open(root + "/" + rel);
        if (!f) { if (err) *err = "cannot open " + root + "/" + rel; return false; }
        return true;
    };
    std::ifstream fi, fc;
    if (!open("mav0/imu0/data.csv", fi) || !open("mav0/cam0/data.csv", fc)) return false;
    std::string line;
    double last = -1;
    while (std::getline(fi, line)) {
        if (line.empty() || line[0] == '#') continue;
        for (char& c : line) if (c == ',') c = ' ';
        std::istringstream ls(line);
        long long ns; ImuData d;
        if (!(ls >> ns >> d.w[0] >> d.w[1] >> d.w[2] >> d.a[0] >> d.a[1] >> d.a[2])) continue;
        d.t = (double)(ns / 1000000000LL) + 1e-9 * (double)(ns % 1000000000LL);   // ros::Time::toSec() of the message stamp
        d.dt = last < 0 ? 0.0 : d.t - last;                     // rvio_mono.cc:97-106
        last = d.t;
        out->imu.push_back(d);
    }
    while (std::getline(fc, line)) {
        if (line.empty() || line[0] == '#') continue;
        const size_t c = line.find(',');
        if (c == std::string::npos) continue;
        const long long ns = std::atoll(line.substr(0, c).c_str());
        std::string name = trim(line.substr(c + 1));
        out->images.emplace_back((double)(ns / 1000000000LL) + 1e-9 * (double)(ns % 1000000000LL), root + "/mav0/cam0/data/" + name);
    }
    std::sort(out->images.begin(), out->images.end());
    return true;
}

}  // namespace rvio
