// host/rvio_host.hpp — the C++ host side above the C-ABI: the reference's System / InputBuffer / settings reader without
// ROS, OpenCV or Eigen (replay and I/O formats).  The per-frame hot path is ONE call into
// librvio_hip.so (rvio_hip_frame); everything here is plumbing with the reference's semantics:
//   Settings + read_settings   System::System / Tracker / Updater / PreIntegrator / FeatureDetector constructors reading the
//                              OpenCV-YAML settings file (System.cc:44-103, Tracker.cc:37-90, Updater.cc:38-69,
//                              PreIntegrator.cc:30-48, FeatureDetector.cc:28-52; keys: config/rvio_euroc.yaml)
//   InputBuffer                InputBuffer.cc:29-81 (time-sorted FIFOs, GetMeasurements)
//   System::MonoVIO            System.cc:172-436: static-start detection and initialisation gate (:185-250), then the timed
//                              body (:253-367) = rvio_hip_frame, then the pose line of stamped_pose_ests.dat (:369-374)
//   read_image / AslDataset    EuRoC ASL folder: mav0/cam0/data.csv + data/*.png (8-bit gray; also binary PGM),
//                              mav0/imu0/data.csv  [ns, wx, wy, wz, ax, ay, az]
// Unlike the reference, sensor packets are owned by value (upstream never frees them).
#pragma once
#include <cstdint>
#include <deque>
#include <list>
#include <string>
#include <utility>
#include <vector>

#include "../include/rvio_hip.h"

namespace rvio {

struct ImuData {          // InputBuffer.h:35-51
    double w[3], a[3];
    double t, dt;
};
struct ImageData {        // InputBuffer.h:53-63 (cv::Mat -> packed bytes, `channels` interleaved samples per pixel: 1, 3 or 4)
    std::vector<uint8_t> px;
    int width = 0, height = 0;
    int channels = 1;
    double t = 0;
    int bits = 8;         // bits per sample: 8, or 16 (two bytes per sample in host byte order, as a cv::Mat of CV_16U holds them)
};
// Tracker::track's "Convert to gray scale" (Tracker.cc:182-196): cvtColor CV_RGB2GRAY / CV_BGR2GRAY (3 channels) or the RGBA / BGRA forms
// (4 channels, alpha ignored) on 8-bit data = OpenCV's fixed-point  (R 4899 + G 9617 + B 1868 + 8192) >> 14.  In place; 1 channel: no-op.
// The host form of what the library does on the device (rvio_hip_set_image_format: System::MonoVIO hands colour images over as they are);
// kept for callers that want the gray image itself (rvio_replay --check-image).
void to_gray(ImageData* im, bool is_rgb);
// What the reference's node does in front of all that, cv_bridge::toCvShare(msg, MONO8) (rvio_mono.cc:64), for any rvio_pixel_format: 16-bit samples
// ("gray at 16 bits, then 16 -> 8": (v + 128) / 257) and Bayer mosaics (cvtColor's bilinear COLOR_Bayer*2GRAY, borders replicated) besides the
// 8-bit formats above.  The host form of the device's arithmetic: it compiles the kernels' own header (r-vio_amd/csrc/raw.h).  In place; false
// with a message when the format does not fit the image (channels, bit depth, a mosaic smaller than 3 x 3).
bool to_gray(ImageData* im, int format, std::string* err);
// a ROS encoding name (mono8, mono16, rgb8 ... bgra16, bayer_rggb8 ... bayer_grbg16) as rvio_pixel_format; -1: unknown
int encoding_format(const std::string& name);

struct Settings {
    rvio_config cfg;              // everything the hot path needs
    double cam_time_offset = 0;   // Camera.nTimeOffset
    int record_outputs = 0;       // INI.RecordOutputs
    int is_rgb = 0;               // Camera.RGB (Tracker.cc:64-65): channel order of a 3 / 4-channel image, 1 = RGB(A), 0 = BGR(A)
    std::string encoding;         // Camera.Encoding (optional): sensor_msgs' name of what the camera delivers — the only way to declare a Bayer mosaic
    // Standstill.* (all optional; no reference counterpart): Standstill.Enable: 1 switches the device-side standstill detector and its zero-velocity
    // update on (rvio_hip_set_standstill); .SigmaA .SigmaW .ImuThr .DispThrPx .MinPairs .SigmaV .SigmaBg .BiasRows .Gate override the members of
    // rvio_standstill_config_default, a missing key keeps its default.  Enable: 0 or absent: the host does the calls it did before the keys existed
    int standstill_enable = 0;
    rvio_standstill_config standstill;
    // Meas.Iterations (1 .. RVIO_MEAS_MAX_ITERS) and Meas.Tolerance (>= 0) — optional; no reference counterpart: the fix, past-fix, rel and map
    // measurements relinearised on the device (rvio_hip_set_meas_iterations).  Absent or 1: the single update, and the calls the host did before
    int meas_iterations = 1;
    double meas_tolerance = 0.0;
    std::vector<std::string> missing;   // keys the reference reads (cv::FileStorage would yield 0 for them) that the file does not hold:
                                        // they keep the EuRoC defaults here, and the caller is told (rvio_replay prints them)
};
// Parses the OpenCV-YAML (1.0) subset the reference's settings files use: "Key: scalar" lines, '#' comments and
// "Key: !!opencv-matrix" blocks (rows / cols / dt / data: [ ... ]).  Missing keys keep the EuRoC defaults.
bool read_settings(const std::string& path, Settings* out, std::string* err);
bool parse_settings(const std::string& text, Settings* out, std::string* err);
// The rvio_pixel_format of an image under these settings: Camera.Encoding when it is set — an error when it contradicts the image's channel count
// or bit depth —, else what follows from channels, bit depth and Camera.RGB.  -1 with a message.
int image_format(const ImageData& im, const Settings& s, std::string* err);

class InputBuffer {       // InputBuffer.cc:29-81
public:
    void PushImuData(const ImuData& d);
    void PushImageData(ImageData&& d);
    // false if there is no image, not enough IMU data yet, or fewer than 2 samples precede the image
    bool GetMeasurements(double time_offset, ImageData* image, std::vector<ImuData>* imus);
    size_t images() const { return img_.size(); }
    size_t imus() const { return imu_.size(); }
private:
    std::list<ImuData> imu_;
    std::list<ImageData> img_;
};

struct PoseLine { double t, p[3], q[4]; };   // System.cc:369-374: timestamp pGk(3) qkG(4)

// one line of a --fix file
struct FixRow { double t = 0; int kind = 0; rvio_fix fix{}; };
// A fix file is text, one fix per line, blank lines and '#' lines skipped, fields separated by blanks or commas:
//     t position x y z  sx sy sz  [lx ly lz]
//     t attitude qx qy qz qw  sx sy sz
//     t pose     x y z  qx qy qz qw  sx sy sz  srx sry srz  [lx ly lz]
//     t gravity  ax ay az  sx sy sz
// t: seconds, on the clock of the image stamps; kind: the word or its number (0 .. 3); sigma: one per axis, rad for the attitude, all > 0; the
// lever is optional.  A malformed line — an unknown kind, a wrong field count, a field that is no finite number, a sigma <= 0, a quaternion off
// unit length by more than 1e-6 — is an error that names the line: "<name>:<line number>: <why>: <the line>".
bool parse_fixes(const std::string& text, const std::string& name, std::vector<FixRow>* out, std::string* err);
bool read_fixes(const std::string& path, std::vector<FixRow>* out, std::string* err);
// The record of each kind, as parse_fixes fills it too: the members a kind does not use are 0; lever: nullptr for none
rvio_fix position_fix(const double p[3], const double sigma[3], const double* lever);
rvio_fix attitude_fix(const double q[4], const double sigma[3]);
rvio_fix pose_fix(const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever);
rvio_fix gravity_fix(const double a[3], const double sigma[3]);
// Where a fix stamped t falls among the image stamps of the frames the clone window still reaches (newest first, stamps[a] = the frame of age a):
// FIX_AGE_NOW: at or past the newest composed image (or no frame yet) — fuse at the current state; FIX_AGE_TOO_OLD: older than the oldest frame —
// drop; FIX_AGE_PAST: (age, frac) for rvio_hip_update_fix_past.  interpolate (POSITION): stamps[age + 1] < t <= stamps[age], frac =
// (stamps[age] - t) / (stamps[age] - stamps[age + 1]) in [0, 1), snapped onto a frame within kFixAgeSnap of it.  Otherwise (ATTITUDE, POSE: no
// attitude interpolation) the NEAREST frame, frac = 0 — exact for a fix derived from an image, off by up to half a frame of motion for one that is not.
enum { FIX_AGE_TOO_OLD = -1, FIX_AGE_PAST = 0, FIX_AGE_NOW = 1 };
struct FixAge { int where = FIX_AGE_NOW; int age = 0; double frac = 0.0; };
constexpr double kFixAgeSnap = 1e-6;
FixAge resolve_fix_age(const std::vector<double>& stamps, double t, bool interpolate);

// one line of a --rel file: a delta pose between the instants t_old < t_new (rvio_hip_update_rel)
struct RelRow { double t_new = 0, t_old = 0; int kind = 0; rvio_fix meas{}; };
// A rel file is text like a fix file, one relative-pose measurement per line:
//     t_new t_old position dx dy dz  sx sy sz  [lx ly lz]
//     t_new t_old attitude qx qy qz qw  sx sy sz
//     t_new t_old pose     dx dy dz  qx qy qz qw  sx sy sz  srx sry srz  [lx ly lz]
// kind: the word or its number (16 .. 18, RVIO_REL_*); d: the displacement of the sensed point from t_old to t_new in the axes of the IMU frame at
// t_old; q: the quaternion rotating the IMU frame at t_old into the one at t_new (JPL xyzw); sigmas and lever as in a fix file.  A malformed line
// — also one with t_new <= t_old — is an error that names the line: "<name>:<line number>: <why>: <the line>".
bool parse_rels(const std::string& text, const std::string& name, std::vector<RelRow>* out, std::string* err);
bool read_rels(const std::string& path, std::vector<RelRow>* out, std::string* err);
// Which two frames of the window a pair of stamps means (stamps newest first, as for resolve_fix_age): BOTH go to the NEAREST frame (no
// interpolation between frames); t_new at or past the newest composed image is that image (age 0).  ok = false — the pair is dropped — when the
// older stamp has left the window (or the newer one has), when the two resolve to one frame, and when nothing is composed yet
struct RelSpan { bool ok = false; int age_new = 0, age_old = 0; };
RelSpan resolve_rel_span(const std::vector<double>& stamps, double t_new, double t_old);

// one line of a --map file: the observation of a known world point in the image stamped t (rvio_hip_update_map)
struct MapRow { double t = 0; rvio_map_obs obs{}; };
// A map file is text like a fix file, one observation per line:
//     t x y z u v sigma
// t: the stamp of the image the match was made in; x y z: the point in the filter's world frame (anchored at the first IMU frame and, with
// Initialization.EnableAlignment, turned to be gravity-aligned — the frame of the pose line: aligning a map frame to it is the caller's job); u v: the observation, raw pixels or undistorted normalised coordinates (rvio_replay --map-units); sigma > 0 in the units
// of u v.  Lines of one stamp form a group, fused together.  A malformed line is an error that names the line.
bool parse_map(const std::string& text, const std::string& name, std::vector<MapRow>* out, std::string* err);
bool read_map(const std::string& path, std::vector<MapRow>* out, std::string* err);
// Which frame of the window a stamp means (stamps newest first, as for resolve_fix_age): the NEAREST frame — exact for a match made in an image,
// which is what a map observation is; at or past the newest composed image: that image (age 0).  ok = false — the group is skipped — when the
// stamp is older than the window, and when nothing is composed yet
struct MapAge { bool ok = false; int age = 0; };
MapAge resolve_map_age(const std::vector<double>& stamps, double t);
// (first, count) of the successive calls n points are fused in: RVIO_MAP_MAX_POINTS per call, the rest in the last one
std::vector<std::pair<int, int>> map_calls(int n);

class System {
public:
    System(const Settings& s, int device);
    ~System();
    System(const System&) = delete;
    System& operator=(const System&) = delete;
    bool ok() const { return h_ != nullptr; }
    const std::string& error() const { return err_; }

    void PushImuData(const ImuData& d) { buf_.PushImuData(d); }          // System::PushImuData, System.h:60
    void PushImageData(ImageData&& d) { buf_.PushImageData(std::move(d)); }
    // System::MonoVIO.  Returns 1 if a frame went through the filter (pose valid), 0 if nothing was processed or the filter is
    // still waiting for motion, <0 on a library error.
    int MonoVIO(PoseLine* pose);
    // INI.RecordOutputs (System.cc:81-88): open <dir>/stamped_pose_ests.dat and <dir>/time_cost.dat (upstream: the package directory).
    // While recording, a frame runs stage by stage like upstream — Tracker::track, then propagate / update / augment / compose, the host
    // waiting behind each — so that the two spans of time_cost.dat (System.cc:254-260,367: t2-t1 and t3-t2, milliseconds) mean what they
    // mean there; without it the frame is one pipelined rvio_hip_frame call.  No-op unless the settings ask for it (or `force`).
    bool record_to(const std::string& dir, bool force = false);
    // Updater::update's landmark cloud (Updater.cc:78-87,430-448,458: what the reference publishes on /rvio/landmarks): enables it on the
    // handle (rvio_hip_set_landmarks) and appends the cloud to `path` behind every frame whose update stamp is new — one line per point,
    // format_landmarks.  The settings file has no key for it.
    bool record_landmarks_to(const std::string& path);
    // The 3 x 3 covariance of every cloud point (rvio_hip_set_landmark_cov; it switches the cloud on if that is off): appends the records of
    // the cloud to `path` behind every frame whose update stamp is new — one line per point, format_landmark_cov.  The file of
    // record_landmarks_to keeps its format.  The settings file has no key for it.
    bool record_landmark_cov_to(const std::string& path);
    // What the reference publishes every frame as nav_msgs::Odometry and appends to its nav_msgs::Path (System.cc:402-434): enables the
    // handle's odometry ring (rvio_hip_set_odometry, `ring` records) and keeps the image timestamps by seq on the host.  The ring is read
    // with ONE rvio_hip_get_odometry whenever ring / 2 frames are outstanding and once more at the end (flush_odometry, also run by the
    // destructor): the pipelined frame is no longer drained once per image for its pose.  One line per frame, format_odometry.
    bool record_odometry_to(const std::string& path, int ring = 256);
    int flush_odometry();         // 0, or -1 on a library error (error())
    // The fixed-lag smoothed trajectory: enables the handle's smoothed-odometry ring (rvio_hip_set_smoothed_odometry, `ring` records, the frame
    // `lag` images back behind every frame) and keeps the image stamps by frame count on the host: a record's stamp is that of the image it
    // describes, `lag` frames before the one it was written behind.  Read like the odometry ring (flush_smoothed, also run by the destructor).
    // One line per record, format_smoothed: the layout of the odometry file.
    bool record_smoothed_to(const std::string& path, int lag, int ring = 256);
    int flush_smoothed();         // 0, or -1 on a library error (error())
    // A pose-graph back end's between-factors: enables the handle's edge-odometry ring (rvio_hip_set_edge_odometry, `ring` records, the edge
    // between the frames age_new < age_old images back behind every frame) and keeps the image stamps by frame count on the host: a record is
    // written with the stamps of the two images it connects.  Read like the smoothed ring (flush_edges, also run by the destructor).  One line
    // per record, format_edge.
    bool record_edges_to(const std::string& path, int age_new, int age_old, int ring = 256);
    int flush_edges();            // 0, or -1 on a library error (error())
    // A dense trajectory: one pose per IMU sample (200 Hz against the 20 Hz of stamped_pose_ests.dat), the pose line MonoVIO would write if an
    // image arrived right behind that sample and ran no update.  Enables the handle's IMU-rate ring (rvio_hip_set_imu_odometry, `ring` samples)
    // and reads it with ONE rvio_hip_get_imu_odometry whenever ring / 2 samples are outstanding and once more at the end
    // (flush_imu_odometry, also run by the destructor): no frame is drained for it.  One line per sample, format_imu_odometry.  A read that
    // returns fewer records than are outstanding — the ring was too small for the samples between two reads and has overwritten some — is an
    // error (MonoVIO / flush_imu_odometry return -1, error() names the counts): the file never misses lines silently.
    // with_cov: the handle's covariance ring runs beside it (rvio_hip_set_imu_odometry_cov) and every line carries format_imu_odometry_cov's 27
    // columns behind its 11; without it the file is what it was before the covariance ring existed
    bool record_imu_odometry_to(const std::string& path, int ring = 4096, bool with_cov = false);
    int flush_imu_odometry();     // 0, or -1 on a library error or on records lost to a ring too small (error())
    // the handle's sticky device-side flags (rvio_frame_info.reserved[0]: 1 singular pivot, 2 a track dropped, 4 a stage counter timed out,
    // 8 a non-positive gate pivot; 0 = none) — waits for everything in flight, so a replay reads it once at its end.  -1: the query failed.
    int device_flags();
    // The auxiliary measurement update (rvio_hip_update_aux): what is not a camera track — wheel odometry, standing still, a speed-over-ground
    // sensor — fused into the filter on the device, behind the last frame handed over and ahead of the next; no frame is drained for it.
    // update_aux: any measurement the caller has linearised, m <= RVIO_AUX_MAX_ROWS rows over state_dim() columns.  velocity: the velocity in
    // the IMU frame {Rk} (state slot v, error columns 15..17) was measured as v, each axis with standard deviation sigma; zero_velocity: it
    // was 0.  gate: apply only if the measurement passes the 95 % chi-square test the features pass.  0, or -1 with error().
    int update_aux(const rvio_aux_meas& meas);
    int zero_velocity(double sigma, bool gate);
    int velocity(const double v[3], double sigma, bool gate);
    // Standstill.Enable: 1: MonoVIO calls rvio_hip_standstill(the IMU samples of the frame, apply = 1) behind every frame once the filter is
    // initialised — the device decides, the host sees nothing.  record_standstill_to: additionally read the record of every frame through
    // rvio_hip_get_standstill (its wait for the filter stream is the only synchronisation this adds, and only when the file is asked for) into a
    // host-side vector, written ONCE at the end (flush_standstill, also run by the destructor): one line per frame, format_standstill
    bool record_standstill_to(const std::string& path);
    int flush_standstill();       // 0, or -1 when the file cannot be written (error())
    bool standstill_enabled() const { return ss_on_; }
    // Absolute fixes (rvio_hip_update_fix): a world-frame position (GNSS / RTK, UWB, a motion-capture marker), attitude or pose (motion capture,
    // a fiducial, a relocalisation result), or the accelerometer at rest, linearised on the device at the state the call finds — no state is
    // read back.  Positions and quaternions in the frame and convention of the pose line (PoseLine: pGk, qkG JPL xyzw; the world frame is the
    // first IMU frame, NOT gravity-aligned); sigma: per axis (rad for an attitude); lever: the sensed point in the IMU frame, nullptr = the IMU
    // itself; gate: the 95 % chi-square test.  0, or -1 with error().
    int update_fix(int kind, const rvio_fix& fix, bool gate);
    int fix_position(const double p[3], const double sigma[3], const double* lever, bool gate);
    int fix_attitude(const double q[4], const double sigma[3], bool gate);
    int fix_pose(const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate);
    int fix_gravity(const double a[3], const double sigma[3], bool gate);
    // fixes with time stamps (rvio_replay --fix): MonoVIO fuses each one behind the first frame whose image stamp is >= its t, ahead of that
    // frame's pose read-back — AT THAT FRAME'S STATE, not at t: bridging the gap (propagating to the fix's stamp) is not done.  Rows are sorted by t
    // latency >= 0 (rvio_replay --fix-latency): a fix becomes available behind the first frame whose stamp is >= its t + latency and is fused AT ITS
    // OWN t through the _at calls below; < 0: as described above
    void queue_fixes(std::vector<FixRow> rows, bool gate, double latency = -1.0);
    long fixes_applied() const { return (long)fx_next_; }
    // Delayed fixes (rvio_hip_update_fix_past): the same measurements with the time t they were taken at, on the clock of the image stamps.  The
    // System keeps the stamp of every frame the clone window still reaches; t is resolved against them (resolve_fix_age above): a POSITION is
    // interpolated between the two frames around t, an ATTITUDE or POSE goes to the nearest frame (exact for image-derived fixes, otherwise off by
    // up to half a frame of motion); a t at or past the newest composed image falls through to the calls above (fused at the current state: the gap
    // to a stamp newer than the last image is not bridged); a t older than the window is dropped and counted.  0, or -1 with error().
    int update_fix_at(double t, int kind, const rvio_fix& fix, bool gate);
    int fix_position_at(double t, const double p[3], const double sigma[3], const double* lever, bool gate);
    int fix_attitude_at(double t, const double q[4], const double sigma[3], bool gate);
    int fix_pose_at(double t, const double p[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate);
    long fixes_dropped() const { return fx_dropped_; }
    // Relative-pose measurements (rvio_hip_update_rel): the delta pose of the IMU between the instants t_old < t_new, on the clock of the image
    // stamps — a wheel-odometry integrator's increment, a scan matcher's or a second visual odometry's result, a loop closure inside the window —
    // linearised on the device against the clones between the two frames; no state is read back.  Both stamps go to the NEAREST frame the window
    // still reaches (resolve_rel_span above; t_new at or past the newest composed image is that image): exact for deltas between images, off by
    // up to half a frame of motion at either end otherwise.  A pair whose older stamp has left the window, or whose stamps resolve to one frame,
    // is dropped and counted.  d: the displacement of the sensed point from t_old to t_new in the IMU axes at t_old; q: the quaternion rotating
    // the IMU frame at t_old into the one at t_new; kind: RVIO_REL_*.  0, or -1 with error().
    int update_rel_at(double t_new, double t_old, int kind, const rvio_fix& meas, bool gate);
    int rel_position_at(double t_new, double t_old, const double d[3], const double sigma[3], const double* lever, bool gate);
    int rel_attitude_at(double t_new, double t_old, const double q[4], const double sigma[3], bool gate);
    int rel_pose_at(double t_new, double t_old, const double d[3], const double q[4], const double sigma_p[3], const double sigma_q[3], const double* lever, bool gate);
    long rels_dropped() const { return rl_dropped_; }
    // measurements with time stamps (rvio_replay --rel): MonoVIO fuses each one behind the first frame whose image stamp is >= its t_new, ahead of
    // that frame's pose read-back.  Rows are sorted by t_new
    void queue_rels(std::vector<RelRow> rows, bool gate);
    long rels_applied() const { return (long)rl_next_; }
    // Map landmarks (rvio_hip_update_map): n observations of known world points made in the image stamped t, on the clock of the image stamps —
    // a surveyed marker, a fiducial's corners, 2D-3D matches against a prior map — linearised on the device against the camera pose the window
    // holds for the NEAREST frame (resolve_map_age above); gate_each: every point behind its own 95 % chi-square gate (no stack gate).  The gate
    // protects a consistent filter from wrong matches; a filter that has drifted further than its covariance admits refuses correct matches
    // too, and a caller who trusts the matches (a relocalisation) switches it off.  More
    // than RVIO_MAP_MAX_POINTS points are fused in successive calls (map_calls): sequential updates of independent measurements are valid.  A
    // stamp older than the window is skipped and counted (maps_skipped, and the stamps themselves in map_skipped_stamps).  units: RVIO_MAP_*.
    // 0, or -1 with error().
    int map_points_at(double t, const rvio_map_obs* pts, int n, int units, bool gate_each = true);
    long maps_skipped() const { return (long)mp_skipped_.size(); }
    const std::vector<double>& map_skipped_stamps() const { return mp_skipped_; }
    // observations with time stamps (rvio_replay --map): MonoVIO fuses each group of one stamp behind the first frame whose image stamp is >= its
    // t + latency (matches arrive late: latency >= 0 seconds), AT ITS OWN t.  Rows are sorted by t.  gate_each as above (rvio_replay --map-gate)
    void queue_map(std::vector<MapRow> rows, int units, double latency, bool gate_each);
    long map_groups_applied() const { return mp_groups_; }
    // the iterated update of every fix / past-fix / rel / map measurement from here on (rvio_hip_set_meas_iterations; rvio_replay --meas-iters,
    // --meas-tol; the settings keys Meas.Iterations, Meas.Tolerance).  false with error() when the library refuses the values
    bool set_meas_iterations(int max_iters, double tol);
    // what the last such measurement took (rvio_hip_get_meas_iter of instance 0: waits for the filter stream); false with error() before the first
    bool last_meas_iter(rvio_meas_iter* out);
    // columns of an auxiliary H right now: 24 + 6 clones, the clones counted as the library counts them (one per frame behind the first, up
    // to Tracker.nMaxTrackingLength - 1) — no read-back
    int state_dim() const;
    bool recording() const { return rec_; }
    bool is_ready() const { return ready_; }
    int frames_after_init() const { return n_img_; }
    rvio_hip* handle() { return h_; }

private:
    Settings s_;
    rvio_hip* h_ = nullptr;
    std::string err_;
    InputBuffer buf_;
    bool moving_ = false, ready_ = false;
    double wm_[3] = {0, 0, 0}, am_[3] = {0, 0, 0};
    int n_imu_ = 0, n_img_ = 0;
    bool rec_ = false;
    int pix_fmt_ = RVIO_PIX_MONO8;   // the image format the handle was last told (rvio_hip_set_image_format)
    void* f_pose_ = nullptr;      // std::ofstream* (kept out of the header)
    void* f_time_ = nullptr;
    void* f_lm_ = nullptr;        // std::ofstream* of record_landmarks_to
    int lm_last_ = -1;            // frame stamp of the last cloud written
    std::vector<int32_t> lm_feat_;
    std::vector<double> lm_pr_, lm_pw_;
    int write_landmarks(double t);
    void* f_lmc_ = nullptr;       // std::ofstream* of record_landmark_cov_to
    int lmc_last_ = -1;           // frame stamp of the last records written
    std::vector<rvio_landmark_cov> lmc_rec_;
    int write_landmark_cov(double t);
    void* f_od_ = nullptr;        // std::ofstream* of record_odometry_to
    int od_ring_ = 0;
    long long od_seq_ = 0, od_read_ = 0;   // frames handed to the filter since initialisation / records written to the file
    std::deque<double> od_t_;     // image timestamps of the records not yet written: front() belongs to seq od_read_ + 1
    std::vector<rvio_odom> od_buf_;
    int note_odometry(double t);
    void* f_sm_ = nullptr;        // std::ofstream* of record_smoothed_to
    int sm_ring_ = 0, sm_new_ = 0;         // sm_new_: frames handed to the filter since the ring was last read
    long long sm_read_ = 0;       // seq of the last record written to the file
    std::deque<std::pair<int, double>> sm_t_;   // (frame count, image stamp) of the frames no record has described yet, oldest first
    std::vector<rvio_window_pose> sm_buf_;
    int note_smoothed(double t);
    void* f_ed_ = nullptr;        // std::ofstream* of record_edges_to
    int ed_ring_ = 0, ed_new_ = 0;         // ed_new_: frames handed to the filter since the ring was last read
    long long ed_read_ = 0;       // seq of the last record written to the file
    std::deque<std::pair<int, double>> ed_t_;   // (frame count, image stamp) of the frames a coming record may still name, oldest first
    std::vector<rvio_window_edge> ed_buf_;
    int note_edges(double t);
    long long last_seq();
    void* f_io_ = nullptr;        // std::ofstream* of record_imu_odometry_to
    int io_ring_ = 0;
    long long io_seq_ = 0, io_read_ = 0;   // IMU samples handed to the filter since initialisation / up to which the ring has been read
    std::vector<rvio_imu_pose> io_buf_;
    bool io_cov_ = false;         // record_imu_odometry_to(with_cov)
    std::vector<rvio_imu_cov> ioc_buf_;
    int note_imu_odometry(int m);
    bool ss_on_ = false;          // Standstill.Enable and rvio_hip_set_standstill succeeded
    std::string ss_path_;         // record_standstill_to
    std::vector<std::pair<double, rvio_standstill>> ss_recs_;
    int standstill(double t, const rvio_imu* imu, int m);
    std::vector<FixRow> fx_rows_; // queue_fixes, sorted by t
    size_t fx_next_ = 0;          // the first row not yet fused
    bool fx_gate_ = false;
    double fx_latency_ = -1.0;    // queue_fixes: >= 0 = fuse at the fix's own stamp once t + latency has passed
    long fx_dropped_ = 0;         // _at calls older than the window
    std::deque<double> stamps_;   // image stamps of the composed frames the clone window still reaches, newest first
    void note_stamp(double t);
    int apply_fixes(double t);
    std::vector<RelRow> rl_rows_; // queue_rels, sorted by t_new
    size_t rl_next_ = 0;          // the first row not yet handed on
    bool rl_gate_ = false;
    long rl_dropped_ = 0;         // pairs the window no longer holds, or that fall onto one frame
    int apply_rels(double t);
    std::vector<MapRow> mp_rows_; // queue_map, sorted by t
    size_t mp_next_ = 0;          // the first row not yet handed on
    int mp_units_ = RVIO_MAP_NORMALISED;
    double mp_latency_ = 0.0;
    bool mp_gate_ = false;
    long mp_groups_ = 0;          // groups handed to map_points_at
    std::vector<double> mp_skipped_;   // stamps of the groups the window no longer held
    int apply_map(double t);
};

// 8- or 16-bit PNG (non-interlaced; gray, RGB or RGBA: channels in file order = RGB) or binary PGM / PPM (P5 / P6; maxval 255: 8 bits, 256 ..
// 65535: 16 bits).  Both file formats store 16-bit samples big endian; ImageData holds them in host byte order.
bool read_image(const std::string& path, ImageData* out, std::string* err);
bool decode_png_gray8(const uint8_t* data, size_t n, ImageData* out, std::string* err);

struct AslDataset {
    std::vector<std::pair<double, std::string>> images;   // (t [s], absolute path)
    std::vector<ImuData> imu;                             // dt = t - previous t (0 for the first), rvio_mono.cc:97-106
};
bool read_asl(const std::string& root, AslDataset* out, std::string* err);

std::string format_pose(const PoseLine& p);               // one line of stamped_pose_ests.dat, setprecision(19)
// the points of one cloud (rvio_hip_get_landmarks), one line each: t frame feat xw yw zw xr yr zr (world frame, then {Rk} as published), %.19g
std::string format_landmarks(double t, int frame, int n, const int32_t* feat, const double* p_world, const double* p_r);
// the records of one cloud (rvio_hip_get_landmark_cov), one line each: t feat n_obs status p_w[3] cov_w (the 6 entries on and above the diagonal,
// by rows) p_r[3] cov_r (likewise) rho rho_sigma, %.19g (NaN prints as nan)
std::string format_landmark_cov(double t, int n, const rvio_landmark_cov* rec);
// one record of the odometry ring: t seq px py pz qx qy qz qw vx vy vz c00 ... c55 (pose_cov row by row), %.19g
std::string format_odometry(double t, const rvio_odom& r);
// one record of the smoothed-odometry ring in the same layout; the three velocity columns are 0 (the window holds no velocity of a past frame)
std::string format_smoothed(double t, const rvio_window_pose& r);
// one record of the edge-odometry ring: t_new t_old px py pz qx qy qz qw c00 ... c55 (cov row by row), %.19g — p the origin of the newer frame
// in the older, along the older frame's axes; q (JPL, xyzw) rotates the older frame into the newer; cov rows: p, then the rotation error along the
// newer frame's axes under R_true ~ (I - [dth x]) R(q) (rvio_window_edge of include/rvio_hip.h)
std::string format_edge(double t_new, double t_old, const rvio_window_edge& r);
// one record of the IMU-rate ring: t px py pz qx qy qz qw vx vy vz, %.19g (setprecision(19), like stamped_pose_ests.dat)
std::string format_imu_odometry(const rvio_imu_pose& r);
// the same line with the paired covariance record behind it: the 21 entries of pose_cov's upper triangle row by row (c00 c01 ... c05 c11 ... c55, order
// x y z rotX rotY rotZ), then the 6 of vel_cov's (v00 v01 v02 v11 v12 v22), %.19g
std::string format_imu_odometry_cov(const rvio_imu_pose& r, const rvio_imu_cov& c);
// one standstill record: t T disparity n_pairs flags gamma, %.19g
std::string format_standstill(double t, const rvio_standstill& r);
std::string format_time_cost(int n_img, double track_ms, double filter_ms);   // one line of time_cost.dat (System.cc:376-378)

}  // namespace rvio
